// mpcekf_hild.hpp -- hildreth.m for runMPC.m's Np = 5 / Nc = 2 constraint stack, lane per
// problem: the rank-2 sweeps, their per-lane LDS slots and the iterMPC.m:68-95 tail, shared
// by the translation units that launch them (mpcekf_kernels.hip: all switches on;
// mpcekf_switch.hip: a constraint block switched off).  Every piece is templated on the
// switch mask SW (mpcekf_mpc.hpp: row_on); SW_ALL, the default, is the full 23-row stack.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mpcekf_kernels.hpp"
#include "mpcekf_mpc.hpp"

#pragma clang fp contract(off)

namespace mk {

constexpr int NP = 5;                  // compiled horizon (runMPC.m:28)
constexpr int NC = 2;                  // compiled control horizon (runMPC.m:29)
constexpr int NCON = 4 * NC + 3 * NP;  // constraint rows (constraintsMPC.m)

// k_hild: rows of LDS operand prefetch in the fast sweep
#ifndef MPCEKF_HILD_PF
#define MPCEKF_HILD_PF 3
#endif

using Cons = ConsT<NP, NC>;
using MpcSetup = MpcSetupT<NP, NC>;

struct ConsM {
  const Cons &C;
  __device__ __forceinline__ double operator()(int i, int k) const { return mval(C, i, k); }
};
struct DenseM {
  const double (&M)[NCON][NC];
  __device__ __forceinline__ double operator()(int i, int k) const { return M[i][k]; }
};

// Hildreth problem record handed from k_cell to k_hild, SoA [field][cell].
enum { PB_E = 0, PB_F = PB_E + NC * NC, PB_HV = PB_F + NC, PB_HE = PB_HV + NP, PB_HS = PB_HE + NP,
       PB_GAM = PB_HS + NP, PB_ERR = PB_GAM + NCON, PB_RU = PB_ERR + NP, PB_UK1 = PB_RU + 1, PB_N = PB_UK1 + 1 };

static_assert(PB_N == PROB_DOUBLES, "problem record size");

// hildreth.m:17-46.  H(i,:)*lambda is summed in orc_hildreth's defined order: four
// interleaved partial sums p_q (terms j = q mod 4, each from +0 in ascending j),
// combined as (p0 + p1) + (p2 + p3).  None of these sums can be -0.
//
// X = E\M' is kept for the 15 Toeplitz rows plus three solves for the constant
// current rows: X(-b) = -X(b) exactly under round-to-nearest; the sign of a
// zero in those X entries cannot reach the sweep (it only feeds products added to
// sums that are never -0, and their diagonal H_ii = E^-1_00 > 0).
struct XS {
  double a[NC], b[NC], c[NC];        // E\[1;0], E\[1;1], E\[0;1]
  double t[3 * NP][NC];              // E\M(i,:)' for the V / eta / SOC rows
};
__device__ __forceinline__ double xval(const XS &X, int j, int k) {
  switch (j) {  // rows of [Cu; -Cu; I; -I] for NC == 2
    case 0: return X.a[k];
    case 1: return X.b[k];
    case 2: return -X.a[k];
    case 3: return -X.b[k];
    case 4: return X.a[k];
    case 5: return X.c[k];
    case 6: return -X.a[k];
    case 7: return -X.c[k];
    default: return X.t[j - 4 * NC][k];
  }
}

// The switch mask on this stack (mpcekf_mpc.hpp).  Rows keep their all-on number i, so
// hslot / hneg / mzero and the storage slots are the same for every mask; a row of a disabled
// block is skipped in each unrolled loop (a constant of the loop), and its X entries, LDS
// slots, K, lambda and gamma are never read.
template <int SW>
__device__ __forceinline__ constexpr bool ron(int i) { return row_on<NP, NC, SW>(i); }
template <int SW>
constexpr int NCON_SW = ncon_sw<NP, NC, SW>();

// X = E\M' in compressed form (hildreth.m:25); fin = every X and M entry finite.
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_x(const Cons &Cn, const double E[NC][NC], XS &Xs, bool &fin) {
  ConsM Mf{Cn};
  double R[NC][NC];
  bool ok = chol_n<NC>(E, R);
  if constexpr ((SW & SW_CUR) != 0) {
    double b1[NC] = {1.0, 0.0}, b2[NC] = {1.0, 1.0}, b3[NC] = {0.0, 1.0};
    mldiv_spd<NC>(E, R, ok, b1, Xs.a);
    mldiv_spd<NC>(E, R, ok, b2, Xs.b);
    mldiv_spd<NC>(E, R, ok, b3, Xs.c);
  }
#pragma unroll
  for (int i = 4 * NC; i < NCON; ++i) {
    if (!ron<SW>(i)) continue;
    double b[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) b[k] = Mf(i, k);
    mldiv_spd<NC>(E, R, ok, b, Xs.t[i - 4 * NC]);
  }
  fin = true;
#pragma unroll
  for (int j = 0; j < NCON; ++j) {
    if (!ron<SW>(j)) continue;
    fin = fin && isfinite(xval(Xs, j, 0)) && isfinite(xval(Xs, j, 1)) && isfinite(Mf(j, 0)) && isfinite(Mf(j, 1));
  }
}

// Per-lane LDS of the rank-2 sweeps: the 18 distinct X(:,i) (rows 0-7 of
// [Cu; -Cu; I; -I] are +-a, +-b, +-c) and the 18 distinct (H_ii, 1/H_ii) pairs (H_ii of
// a negated row is bit-identical: (-1)(-x) = x, and its 0 * (-x) term only meets
// a nonzero sum or +0).  Layout [slot][64 lanes] double2: every read is one
// conflict-free ds_read_b128 per wave.  1/H_ii is the correctly rounded reciprocal of hild_step.
constexpr int HS_X = 3 + 3 * NP, HS_SLOTS = 2 * HS_X;
constexpr int HILD_LDS_PER_WAVE = HS_SLOTS * 64 * 16;  // bytes
__device__ __forceinline__ constexpr int hslot(int i) {
  return i >= 8 ? 3 + (i - 8) : (i == 1 || i == 3) ? 1 : (i == 5 || i == 7) ? 2 : 0;
}
__device__ __forceinline__ constexpr bool hneg(int i) { return i == 2 || i == 3 || i == 6 || i == 7; }
// The first row of each Toeplitz block is (H(0), 0): all zero when H(0) = 0, as for the
// SOC block (predMat: G(1,1) = +0), so its H_ii may be 0; 1/H_ii is then +-inf and hild_step's
// product gives x / +-0's inf / NaN by IEEE without a select.
__device__ __forceinline__ double2 hx(const double2 *hl, int i) {  // X(:,i)
  const double2 x = hl[hslot(i) * 64];
  return hneg(i) ? make_double2(-x.x, -x.y) : x;
}
__device__ __forceinline__ double2 hh(const double2 *hl, int i) {  // (H_ii, 1/H_ii)
  return hl[(HS_X + hslot(i)) * 64];
}
__device__ __forceinline__ double2 *hild_lane_lds(double2 *base) {  // blocks of 256 threads
  return base + (threadIdx.x >> 6) * (HS_SLOTS * 64) + (threadIdx.x & 63);
}
// Fills the lane's slots; returns whether every H_ii is in hild_step's reciprocal domain
// (hild_rok: 0 or [2^-1020, 2^1020]), where a row is min(t (1/H_ii), lambda_i).
template <int SW = SW_ALL>
__device__ __forceinline__ bool hild_stage(const Cons &Cn, const XS &Xs, double2 *hl) {
  ConsM Mf{Cn};
  bool yok = true;
#pragma unroll
  for (int sl = 0; sl < HS_X; ++sl) {
    const int i = sl == 0 ? 0 : sl == 1 ? 1 : sl == 2 ? 5 : 8 + (sl - 3);  // representative row
    if (!ron<SW>(i)) continue;  // a disabled block's slots stay unwritten and unread
    const double x0 = xval(Xs, i, 0), x1 = xval(Xs, i, 1);
    const double hii = (0.0 + Mf(i, 0) * x0) + Mf(i, 1) * x1;  // orc_hildreth's H(i,i)
    yok = yok && hild_rok(hii);
    hl[sl * 64] = make_double2(x0, x1);
    hl[(HS_X + sl) * 64] = make_double2(hii, 1.0 / hii);  // the oracle's 1.0 / hii (IEEE)
  }
  return yok;
}
__device__ __forceinline__ void hild_unstage(const double2 *hl, XS &Xs) {
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    Xs.a[k] = k ? hl[0].y : hl[0].x;
    Xs.b[k] = k ? hl[64].y : hl[64].x;
    Xs.c[k] = k ? hl[128].y : hl[128].x;
  }
#pragma unroll
  for (int i = 0; i < 3 * NP; ++i) {
    const double2 x = hl[(3 + i) * 64];
    Xs.t[i][0] = x.x;
    Xs.t[i][1] = x.y;
  }
}

// One rank-2 sweep (orc_hildreth, finite X and M): v = X*lambda from +0 at the sweep
// start (fma, ascending j), t_i = fma(M_i1, v1, fma(M_i0, v0, K_i)),
// m = min(t_i (1/H_ii), lambda_i), d = -m, lambda_i -= m (hild_step with every H_ii in its
// domain and lambda finite), v += X(:,i) * d by fma.  A row's dependent chain is t (2 fma) ->
// q -> min -> v: 5 operations (10 with round 5's division); the new lambda_i is beside it and
// can take lambda_i's register (no rotation of the 23 lambdas at the sweep's end).
// The fast form: straight line, no frozen lanes (the caller keeps a converged lane's
// lambda aside).  It reports max |d| (the reference's inf-norm test, hildreth.m:39) and
// whether v ended finite (false once any d was not finite: inf and NaN stay in v; every
// lambda was finite until then, so each row was hild_step's reciprocal form).
// The constant rows 0-7 ([Cu; -Cu; I; -I]) use 3 of the 18 slots (X: +-a, +-b, +-c; their
// (H_ii, 1/H_ii)): those 6 pairs are held in registers (xr3 / hr3, read back from the
// lane's LDS slots once per solve), so a sweep reads LDS for the 15 Toeplitz rows only.
// At 4 waves per CU in the maxIter window the two ds_read_b128 per row were as long as
// the row's dependent chain.
constexpr int HILD_REG_ROWS = 4 * NC;
__device__ __forceinline__ double2 hx_r(const double2 *hl, const double2 xr3[3], int i) {
  if (i < HILD_REG_ROWS) {
    const double2 x = xr3[hslot(i)];
    return hneg(i) ? make_double2(-x.x, -x.y) : x;
  }
  return hx(hl, i);
}
__device__ __forceinline__ double2 hh_r(const double2 *hl, const double2 hr3[3], int i) {
  return i < HILD_REG_ROWS ? hr3[hslot(i)] : hh(hl, i);
}
// M(i, k) is a structural zero of constraintsMPC.m's M (a constant of the unrolled row loop)
__device__ __forceinline__ constexpr bool mzero(int i, int k) {
  return i < NC ? k > i
       : i < 2 * NC ? k > i - NC
       : i < 3 * NC ? (i - 2 * NC) != k
       : i < 4 * NC ? (i - 3 * NC) != k
       : i < 4 * NC + NP ? k > i - 4 * NC
       : i < 4 * NC + 2 * NP ? k > i - 4 * NC - NP
                             : k > i - 4 * NC - 2 * NP;
}
// v = X*lambda from +0 in ascending j (the sweep-start v of orc_hildreth)
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_v(const double2 *hl, const double2 xr3[3], const double L[NCON], double &v0,
                                       double &v1) {
  v0 = 0.0;
  v1 = 0.0;
#pragma unroll
  for (int j = 0; j < NCON; ++j) {
    if (!ron<SW>(j)) continue;  // ascending over the enabled rows only
    const double2 x = hx_r(hl, xr3, j);
    v0 = __builtin_fma(x.x, L[j], v0);
    v1 = __builtin_fma(x.y, L[j], v1);
  }
}
// (v0, v1): this sweep's start v in, the next sweep's out.  The next sweep's v is summed
// row by row from lambda_i's final value of this sweep (row i is the last to change it),
// the same fmas on the same operands in the same order as hild_v after the sweep, with the
// X(:,i) the row already read.
// With a block switched off the loop runs over the compact stack ci = 0 .. nC - 1 (the
// prefetch ring turns on ci); i = row_full(ci) is still a constant of the unrolled loop.
template <int SW = SW_ALL>
__device__ __forceinline__ void sweep_fast(const Cons &Cn, const double2 *hl, const double2 xr3[3],
                                           const double2 hr3[3], const double K[NCON], double L[NCON],
                                           double &v0, double &v1, double &dmax, bool &vfin) {
  ConsM Mf{Cn};
  constexpr int NCS = NCON_SW<SW>;
  asm volatile("" ::: "memory");  // reload the LDS slots each sweep (no hoisting)
  double u0 = 0.0, u1 = 0.0;
  asm volatile("" ::: "memory");
  // row i's slots are read MPCEKF_HILD_PF rows ahead: ds_read latency (~76 cycles idle,
  // more under load) stays off the chain; one row ahead left ~10 instructions between a
  // read and its use
  constexpr int PF = MPCEKF_HILD_PF;
  double2 xq[PF], hq[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    xq[p] = hx_r(hl, xr3, row_full<NP, NC, SW>(p < NCS ? p : NCS - 1));
    hq[p] = hh_r(hl, hr3, row_full<NP, NC, SW>(p < NCS ? p : NCS - 1));
  }
#pragma unroll
  for (int ci = 0; ci < NCS; ++ci) {
    const int i = row_full<NP, NC, SW>(ci);
    const double2 xc = xq[ci % PF], hc = hq[ci % PF];
    if (ci + PF < NCS) {
      xq[ci % PF] = hx_r(hl, xr3, row_full<NP, NC, SW>(ci + PF));
      hq[ci % PF] = hh_r(hl, hr3, row_full<NP, NC, SW>(ci + PF));
    }
    // M(i, k) entries that are structural zeros (constraintsMPC.m's Cu / I blocks and the
    // first row of each Toeplitz block) add +-0 to t: dropped here.  Exact for the fast form:
    // with v finite a +-0 term changes at most the sign of a zero t, and -t * (1/H_ii) + L_i
    // is then L_i, or +0 when L_i = +0 (round to nearest: -0 + +0 = +0), or NaN for 1/H_ii
    // infinite, either way; a non-finite v marks the sweep bad in both forms
    double t = K[i];
    if (!mzero(i, 0)) t = __builtin_fma(Mf(i, 0), v0, t);
    if (!mzero(i, 1)) t = __builtin_fma(Mf(i, 1), v1, t);
    const double m = fmin_q(t * hc.y, L[i]);   // fmin / fmax(., fabs) without the canonicalising maxes
    const double nl = L[i] - m;
    dmax = fmax_abs_q(dmax, m);
    L[i] = nl;
    v0 = __builtin_fma(-xc.x, m, v0);   // fma(x, d, v) with d = -m: the same value
    v1 = __builtin_fma(-xc.y, m, v1);
    u0 = __builtin_fma(xc.x, nl, u0);
    u1 = __builtin_fma(xc.y, nl, u1);
  }
  vfin = isfinite(v0) && isfinite(v1);
  v0 = u0;
  v1 = u1;
}

// The exact form for lanes the fast form flagged: plain division, v recomputed from
// lambda after a non-finite d (orc_hildreth), frozen lanes (done) keep lambda.
template <int SW = SW_ALL>
__device__ __forceinline__ void sweep_careful(const Cons &Cn, const double2 *hl, const double K[NCON],
                                              double L[NCON], bool done, double tol, bool &conv) {
  ConsM Mf{Cn};
  auto xv = [&](double &v0, double &v1) {
    v0 = 0.0;
    v1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCON; ++j) {
      if (!ron<SW>(j)) continue;
      const double2 x = hx(hl, j);
      v0 = __builtin_fma(x.x, L[j], v0);
      v1 = __builtin_fma(x.y, L[j], v1);
    }
  };
  asm volatile("" ::: "memory");
  double v0, v1;
  xv(v0, v1);
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    if (!ron<SW>(i)) continue;
    const double2 x = hx(hl, i), hr = hh(hl, i);
    double t = __builtin_fma(Mf(i, 0), v0, K[i]);
    t = __builtin_fma(Mf(i, 1), v1, t);
    const double li = L[i];
    double nl;
    const double ds = hild_step(t, hr.x, hr.y, li, nl);
    if (!(fabs(ds) < tol)) conv = false;
    const double nli = done ? li : nl;
    const double d = done ? 0.0 : ds;
    L[i] = nli;
    if (!isfinite(d)) {
      xv(v0, v1);
    } else {
      v0 = __builtin_fma(x.x, d, v0);
      v1 = __builtin_fma(x.y, d, v1);
    }
  }
}

// The dense sweep for lanes with a non-finite X or M entry (orc_hildreth): H(i,:)*lambda
// as 4 interleaved partial sums combined as (p0 + p1) + (p2 + p3).  The partial sum a term
// joins is its row's index in the compact stack (orc_hildreth's j & 3 runs over nC rows).
template <int SW = SW_ALL>
__device__ __forceinline__ void sweep_dense(const Cons &Cn, const XS &Xs, const double K[NCON], double L[NCON],
                                            bool done, double tol, bool &conv) {
  ConsM Mf{Cn};
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    if (!ron<SW>(i)) continue;
    const double m0 = Mf(i, 0), m1 = Mf(i, 1);
    double p4[4] = {0.0, 0.0, 0.0, 0.0}, hii = 0.0;
#pragma unroll
    for (int j = 0; j < NCON; ++j) {
      if (!ron<SW>(j)) continue;
      const double h = (0.0 + m0 * xval(Xs, j, 0)) + m1 * xval(Xs, j, 1);
      if (j == i) hii = h;
      const int q = row_cidx<NP, NC, SW>(j) & 3;
      p4[q] = p4[q] + h * L[j];
    }
    const double s = (p4[0] + p4[1]) + (p4[2] + p4[3]);
    const double li = L[i];
    const double w = -((K[i] + s) - hii * li) / hii;
    const double nl = w > 0 ? w : 0.0;
    if (!(fabs(nl - li) < tol)) conv = false;
    L[i] = done ? li : nl;
  }
}

// hildreth.m:32-44, lane per problem, in two launches.  Every lane of a wave stays in
// each loop until all are done: on MI355X a wave whose EXEC holds fewer than 16 lanes
// issues FP64 VALU up to 2.6x slower under full-chip load (tools/micro/exec_micro.hip).
// `done` = true makes a lane a passenger from the start (a finite dummy problem,
// nothing kept).  hl = the lane's LDS slots (HILD_LDS_PER_WAVE per wave).
//
// hild_fast (k_hild): the fast rank-2 sweep for lanes with finite X, M, every H_ii in
// hild_step's reciprocal domain and a finite warm start.  Lanes keep sweeping after they
// converge; the lambda they converged with goes to L0 (their warm start is no longer
// needed) and comes back after the loop.  A lane whose sweep ends with a non-finite v,
// and every lane outside the fast form's
// domain, returns `slow` with its warm start intact in L0: every sweep before the
// flag was bit-identical to the exact form, so restarting it with the exact rules
// gives the exact form's result.
// hild_slow (k_hild_slow, only waves holding a slow lane): sweep_careful for finite X
// and M, the dense sweep otherwise.  Kept out of k_hild so that the fast loop's
// register allocation carries none of their pressure (224 VGPRs, no AGPR traffic).
template <int SW = SW_ALL>
__device__ __forceinline__ bool hild_fast(const Cons &Cn, const double E[NC][NC], double L[NCON], int maxIter,
                                          double tol, const double K[NCON], bool done, double2 *hl, double *L0,
                                          int64_t l0_stride, int &nexec) {
  static_assert(NC == 2, "written for Nc = 2");
  bool fin, yok;
  {
    XS Xs;
    hild_x<SW>(Cn, E, Xs, fin);
    yok = hild_stage<SW>(Cn, Xs, hl);
  }
  double2 xr3[3], hr3[3];  // slots 0-2 (the constant rows'), the staged bits
  if constexpr ((SW & SW_CUR) != 0) {
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      xr3[sl] = hl[sl * 64];
      hr3[sl] = hl[(HS_X + sl) * 64];
    }
  }
  nexec = maxIter;
  bool lok = true;
#pragma unroll
  for (int i = 0; i < NCON; ++i)
    if (ron<SW>(i)) lok = lok && isfinite(L[i]);
  bool slow = !done && !(fin && yok && lok);
  bool active = !done && !slow;  // still sweeping for itself
  double v0, v1;
  hild_v<SW>(hl, xr3, L, v0, v1);
#pragma unroll 1
  for (int it = 1; it <= maxIter; ++it) {
    if (__all(!active)) break;
    double dmax = 0.0;
    bool vfin;
    sweep_fast<SW>(Cn, hl, xr3, hr3, K, L, v0, v1, dmax, vfin);
    const bool bad = !vfin;
    const bool conv = dmax < tol;
    const bool newconv = active && !bad && conv;
    if (active && bad) slow = true;
    if (newconv) {
      nexec = it;
#pragma unroll
      for (int i = 0; i < NCON; ++i)
        if (ron<SW>(i)) L0[i * l0_stride] = L[i];
    }
    active = active && !bad && !conv;
  }
  // converged lanes take their lambda back; lanes at maxIter keep their last sweep's
  if (!active && !done && !slow) {
#pragma unroll
    for (int i = 0; i < NCON; ++i)
      if (ron<SW>(i)) L[i] = L0[i * l0_stride];
  }
  return slow;
}

template <int SW = SW_ALL>
__device__ __forceinline__ int hild_slow(const Cons &Cn, const double E[NC][NC], double L[NCON], int maxIter,
                                         double tol, const double K[NCON], bool done, double2 *hl) {
  bool fin;
  XS Xs;
  hild_x<SW>(Cn, E, Xs, fin);
  (void)hild_stage<SW>(Cn, Xs, hl);
  int nexec = maxIter;
  if (__any(fin && !done)) {
    bool cdone = done || !fin;
#pragma unroll 1
    for (int it = 1; it <= maxIter; ++it) {
      if (__all(cdone)) break;
      bool conv = true;
      sweep_careful<SW>(Cn, hl, K, L, cdone, tol, conv);
      if (!cdone && conv) {
        cdone = true;
        nexec = it;
      }
    }
  }
  if (__any(!fin && !done)) {
    bool ddone = done || fin;
#pragma unroll 1
    for (int it = 1; it <= maxIter; ++it) {
      if (__all(ddone)) break;
#pragma unroll
      for (int k = 0; k < NC; ++k) {  // opaque per sweep: no hoisting of the 529 H entries
        if constexpr ((SW & SW_CUR) != 0) { launder(Xs.a[k]); launder(Xs.b[k]); launder(Xs.c[k]); }
#pragma unroll
        for (int i = 0; i < 3 * NP; ++i)
          if (ron<SW>(4 * NC + i)) launder(Xs.t[i][k]);
      }
      bool conv = true;
      sweep_dense<SW>(Cn, Xs, K, L, ddone, tol, conv);
      if (!ddone && conv) {
        ddone = true;
        nexec = it;
      }
    }
  }
  return nexec;
}

// M'*lambda (hildreth.m:46; the caller adds F and solves -E\(.))
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_mtl(const Cons &Cn, const double L[NCON], double Mtl[NC]) {
  ConsM Mf{Cn};
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NCON; ++i)
      if (ron<SW>(i)) s = s + Mf(i, k) * L[i];
    Mtl[k] = s;
  }
}

// ---------------------------------------------------------------------------
// k_hild: hildreth.m + iterMPC.m:68-95 for the cells k_cell flagged
// ---------------------------------------------------------------------------
// The QP record of cell c (PB_*) -> Cons, E and K = M*(E\F) + gamma (hildreth.m:29).
// A disabled block's fields are not read (the record holds +0 there): its Hv / He and K are +0.
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_load(const KState &s, int64_t c, Cons &Cn, double E[NC][NC], double K[NCON]) {
  const int64_t n = s.n;
  const double *pb = s.prob;
  double F[NC], y[NC], R[NC][NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    F[a] = pb[(PB_F + a) * n + c];
#pragma unroll
    for (int b = 0; b < NC; ++b) E[a][b] = pb[(PB_E + a * NC + b) * n + c];
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    Cn.Hv[i] = (SW & SW_V) ? pb[(PB_HV + i) * n + c] : 0.0;
    Cn.He[i] = (SW & SW_ETA) ? pb[(PB_HE + i) * n + c] : 0.0;
    Cn.Hs[i] = pb[(PB_HS + i) * n + c];
  }
  bool ok = chol_n<NC>(E, R);
  mldiv_spd<NC>(E, R, ok, F, y);
  ConsM Mf{Cn};
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    if (!ron<SW>(i)) {
      K[i] = 0.0;
      continue;
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) sum = sum + Mf(i, k) * y[k];
    K[i] = sum + pb[(PB_GAM + i) * n + c];
  }
}

// A finite dummy QP for lanes that only ride along (no QP this step / no queued cell).
__device__ __forceinline__ void hild_dummy(Cons &Cn, double E[NC][NC], double K[NCON]) {
#pragma unroll
  for (int a = 0; a < NC; ++a)
#pragma unroll
    for (int b = 0; b < NC; ++b) E[a][b] = a == b ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) Cn.Hv[i] = Cn.He[i] = Cn.Hs[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NCON; ++i) K[i] = 0.0;
}

// DU = -E\(F + M'*lambda) (hildreth.m:46), then iterMPC.m:75-95 and the outputs.
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_finish(const KState &s, const KIO &io, int64_t c, const Cons &Cn,
                                            const double Mtl[NC], int nexec) {
  const int64_t n = s.n;
  const double *pb = s.prob;
  asm volatile("" : "+v"(pb));  // operands re-read after the sweeps, not kept live across them
  MpcOut o;
  o.nexec = nexec;
  MpcSetup P;
  double rhs[NC], mE[NC][NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    rhs[a] = pb[(PB_F + a) * n + c] + Mtl[a];
#pragma unroll
    for (int b = 0; b < NC; ++b) mE[a][b] = -pb[(PB_E + a * NC + b) * n + c];
  }
  lu_solve_n<NC>(mE, rhs, P.DU);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    P.e[i] = pb[(PB_ERR + i) * n + c];
    P.Cn.Hv[i] = Cn.Hv[i];
    P.Cn.He[i] = Cn.He[i];
    P.Cn.Hs[i] = Cn.Hs[i];
  }
#pragma unroll
  for (int i = 0; i < NCON; ++i) P.Cn.gam[i] = ron<SW>(i) ? pb[(PB_GAM + i) * n + c] : 0.0;
  P.Ru = pb[PB_RU * n + c];
  double uk_1 = pb[PB_UK1 * n + c];
  mpc_finish<NP, NC, SW>(P.Cn, P.e, P.Ru, P.DU, uk_1, o);
  s.uk_1[c] = uk_1;
  if (s.J_fin) { s.J_fin[c] = o.J_fin; s.nviol[c] = o.nviol; }
  cost_out(io, c, o.J_fin, o.nviol, norm_du<NC>(P.DU));
  if (io.uk_out) io.uk_out[c] = o.uk;
  if (io.nexec) io.nexec[c] = o.nexec;
  if (io.mode & MODE_FUSED) {
    s.uk[c] = o.uk;
    if (io.u) io.u[c] = o.uk;
  }
}

// hildreth.m + iterMPC.m:68-95, lane per cell: the fast solve (hild_fast).  Blocks of 256
// lanes (hild_lane_lds); k_hild.  A lane outside the fast form's domain is left to
// k_hild_slow (hild_slow_cell), whose exact-rule path keeps its registers out of the fast
// sweep's allocation (profiles/r04h_ab_inline_slow.txt).  lambda keeps the
// all-on slots in s.lam; a disabled row's slot is neither read nor written (it stays 0).
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_cell(const KCfg &cf, const KState &s, const KIO &io, int64_t c) {
  // every lane of the wave stays in the solve; cells without a QP this step ride
  // along on a finite dummy problem and store nothing
  const bool qp = s.hflag[c] != 0;
  const int64_t n = s.n;
  Cons Cn;
  double E[NC][NC], K[NCON], lam[NCON];
  if (!qp) {
    hild_dummy(Cn, E, K);
#pragma unroll
    for (int i = 0; i < NCON; ++i) lam[i] = 0.0;
  } else {
    hild_load<SW>(s, c, Cn, E, K);
#pragma unroll
    for (int i = 0; i < NCON; ++i) lam[i] = ron<SW>(i) ? s.lam[(size_t)i * n + c] : 0.0;
  }
  extern __shared__ double2 hlds[];
  int nexec;
  const bool slow = hild_fast<SW>(Cn, E, lam, cf.max_hild, cf.hild_tol, K, !qp, hild_lane_lds(hlds), s.lam + c, n, nexec);
  if (__any(slow) && (threadIdx.x & 63) == __builtin_amdgcn_readfirstlane(threadIdx.x & 63))
    atomicAdd(s.hslow, 1);  // one add per wave: k_hild_slow has work
  if (!qp) return;
  if (slow) {  // k_hild_slow finishes it (warm start still in s.lam)
    s.hflag[c] = 2;
    return;
  }
  double Mtl[NC];
  hild_mtl<SW>(Cn, lam, Mtl);
#pragma unroll
  for (int i = 0; i < NCON; ++i)
    if (ron<SW>(i)) s.lam[(size_t)i * n + c] = lam[i];  // iterMPC.m:68
  hild_finish<SW>(s, io, c, Cn, Mtl, nexec);
}
template <int SW = SW_ALL>
__device__ __forceinline__ void hild_slow_cell(const KCfg &cf, const KState &s, const KIO &io, int64_t c) {
  if (c >= s.n) return;
  const bool slow = s.hflag[c] == 2;
  if (!__any(slow)) return;
  const int64_t n = s.n;
  Cons Cn;
  double E[NC][NC], K[NCON], lam[NCON];
  if (!slow) {
    hild_dummy(Cn, E, K);
#pragma unroll
    for (int i = 0; i < NCON; ++i) lam[i] = 0.0;
  } else {
    hild_load<SW>(s, c, Cn, E, K);
#pragma unroll
    for (int i = 0; i < NCON; ++i) lam[i] = ron<SW>(i) ? s.lam[(size_t)i * n + c] : 0.0;
  }
  extern __shared__ double2 hlds[];
  const int nexec = hild_slow<SW>(Cn, E, lam, cf.max_hild, cf.hild_tol, K, !slow, hild_lane_lds(hlds));
  if (!slow) return;
  s.hflag[c] = 1;
  double Mtl[NC];
  hild_mtl<SW>(Cn, lam, Mtl);
#pragma unroll
  for (int i = 0; i < NCON; ++i)
    if (ron<SW>(i)) s.lam[(size_t)i * n + c] = lam[i];
  hild_finish<SW>(s, io, c, Cn, Mtl, nexec);
}

}  // namespace mk
