// mpcekf_kernels.hip -- gfx950 kernels of the batched MPC+EKF control step.
//
// Work mapping (DESIGN.md "Kernels"):
//   k_plant4 quad-per-cell   OB_step.m:188-357 minus the all-model advance
//   k_bulk   block-streaming OB_step.m:278 (bigX = bigA.*bigX + Iapp) and the
//                            all-model EKF time update iterEKF.m:73-84, over the
//                            whole cell batch: the HBM-bound part
//   k_cell   lane-per-cell   iterEKF.m:85-210 (4-corner measurement update),
//                            EKFmatsHandler.m, predMat.m, constraintsMPC.m,
//                            iterMPC.m and hildreth.m for one cell per lane
// The ROM (C/D rows, diag(A), OCP tables) is staged once per workgroup in LDS.
// Arithmetic follows the defined order of oracle/mpcekf_oracle.c (sequential
// sums from +0.0, no contraction, asinh spelled out as dasinh), so results match
// it bit-for-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <type_traits>

#include "mpcekf_kernels.hpp"
#include "mpcekf_mpc.hpp"
#include "mpcekf_hild.hpp"

#pragma clang fp contract(off)

#include "mpcekf_dexp.hpp"  // dexp and dm::LN2_HI / LN2_LO, shared with mpcekf_aging.hip

namespace mk {


// Section timestamps of k_cell for profiling builds (-DMPCEKF_STAMPS); compiled out otherwise.
#ifdef MPCEKF_STAMPS
#define STAMP(i)                                                                          \
  do {                                                                                    \
    if (io.stamps) io.stamps[(size_t)(i) * s.n + c] = (long long)__builtin_amdgcn_s_memtime(); \
  } while (0)
#define STAMPP(i)                                                                                  \
  do {                                                                                             \
    if (s.stamps) s.stamps[(size_t)(12 + (i)) * s.n + c] = (long long)__builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define STAMP(i) \
  do {           \
  } while (0)
#define STAMPP(i) \
  do {            \
  } while (0)
#endif

__device__ __forceinline__ int pk(int r, int c) {
  // packed upper-triangular index, row-major over r <= c
  return r <= c ? r * NX - (r * (r - 1)) / 2 + (c - r) : c * NX - (c * (c - 1)) / 2 + (r - c);
}

// Defined asinh (the plant/EKF overpotential, OB_step.m:333-334, iterEKF.m:400-401,
// EKFmatsHandler.m:88-89).  Neither ocml's nor glibc's asinh is correctly rounded, so
// the kernels and oracle/mpcekf_oracle.c (orc_asinh) both evaluate this spelling: a
// reduction to log(u) + c with u = 2^k m, m in (sqrt(2)/2, sqrt(2)], and the classic
// minimax series in s = f / (2 + f), f = m - 1 (Lg1..Lg7, fdlibm's public
// coefficients).  Only +, -, *, /, sqrt and fma: correctly rounded on both sides.
namespace dm {
constexpr double LN2 = 6.93147180559945286227e-01;
constexpr double LG1 = 6.666666666666735130e-01, LG2 = 3.999999999940941908e-01, LG3 = 2.857142874366239149e-01,
                 LG4 = 2.222219843214978396e-01, LG5 = 1.818357216161805012e-01, LG6 = 1.531383769920937332e-01,
                 LG7 = 1.479819860511658591e-01;
constexpr double SQRT2 = 1.4142135623730951;
// log(u) + c for a finite u >= 1; c is the relative correction (u_true - u) / u
__device__ __forceinline__ double log_core(double u, double c) {
  unsigned long long b = (unsigned long long)__double_as_longlong(u);
  int k = (int)(b >> 52) - 1023;
  double m = __longlong_as_double((long long)((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL));
  if (m > SQRT2) { m = 0.5 * m; k = k + 1; }
  double f = m - 1.0;
  double s = f / (2.0 + f);
  double z = s * s;
  double w = z * z;
  double t1 = w * (LG2 + w * (LG4 + w * LG6));
  double t2 = z * (LG1 + w * (LG3 + w * (LG5 + w * LG7)));
  double R = t2 + t1;
  double hfsq = 0.5 * f * f;
  double dk = (double)k;
  return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + (dk * LN2_LO + c))) - f);
}
}  // namespace dm
__device__ __forceinline__ double dasinh(double x) {
  double a = fabs(x);
  if (!(a < __builtin_inf())) return x + x;  // NaN, +-inf
  if (a < 0x1p-28) return x;
  double t;
  if (a > 0x1p28) {
    t = dm::log_core(a, 0.0) + dm::LN2;
  } else if (a > 2.0) {
    t = dm::log_core(2.0 * a + 1.0 / (sqrt(fma(a, a, 1.0)) + a), 0.0);
  } else {  // log1p(a + a^2 / (1 + sqrt(1 + a^2)))
    double a2 = a * a;
    double xx = a + a2 / (1.0 + sqrt(1.0 + a2));
    double u = 1.0 + xx;
    double c = (xx - (u - 1.0)) / u;
    t = dm::log_core(u, c);
  }
  return x < 0 ? -t : t;
}

// v from the quad lane selected by DPP quad_perm control CTRL.
template <int CTRL>
__device__ __forceinline__ double qperm(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
template <int Q>
__device__ __forceinline__ double qbc(double v) {  // lane Q's v in every lane of the quad
  return qperm<Q | (Q << 2) | (Q << 4) | (Q << 6)>(v);
}
__device__ __forceinline__ double shfl64(double v, int lane) {  // v of lane (runtime), ds_bpermute
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(lane << 2, (int)b);
  const int hi = __builtin_amdgcn_ds_bpermute(lane << 2, (int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__device__ __forceinline__ double tabi(const double *t, int n, double x) {
  if (x != x) return __builtin_nan("");
  double xc = fmin(fmax(x, 0.0), 1.0);
  double tt = xc * (double)(n - 1);
  int i = (int)floor(tt);
  if (i > n - 2) i = n - 2;
  double f = tt - (double)i;
  return t[i] + f * (t[i + 1] - t[i]);
}
// ABI v3 polynomial row (include/mpcekf.h tab_npoly): theta's interval i and s = t - i as
// in tabi, then Horner (fma) over the interval's 6 coefficients (a cubic's upper two are 0),
// read from the global table (L2-resident) as three 16-byte loads.  oracle: tab_poly.
// Horner with explicit fma (correctly rounded here and on the host: oracle tab_poly)
__device__ __forceinline__ double horner6(const double2 c01, const double2 c23, const double2 c45, double s) {
  double v = c45.y;
  v = __builtin_fma(s, v, c45.x);
  v = __builtin_fma(s, v, c23.y);
  v = __builtin_fma(s, v, c23.x);
  v = __builtin_fma(s, v, c01.y);
  return __builtin_fma(s, v, c01.x);
}
__device__ __forceinline__ int tab_interval(int n, double x, double &s) {
  double xc = fmin(fmax(x, 0.0), 1.0);
  double tt = xc * (double)(n - 1);
  int i = (int)floor(tt);
  if (i > n - 2) i = n - 2;
  s = tt - (double)i;
  return i;
}
// one row: interval i's coefficients at c + i * istride
__device__ __forceinline__ double tabp(const double *c, int n, double x, int istride) {
  double s;
  const int i = tab_interval(n, x, s);  // a NaN x: interval 0 (fmax), the NaN selected below
  const double2 *p = reinterpret_cast<const double2 *>(c + (size_t)i * istride);
  const double v = horner6(p[0], p[1], p[2], s);
  return x != x ? __builtin_nan("") : v;
}
// two adjacent rows of interval i (the T bracket): a from c + i * istride, b KPOLY after
__device__ __forceinline__ void tabp2(const double *c, int n, double x, int istride, double &a, double &b,
                                      int ro = KPOLY) {
  double s;
  const int i = tab_interval(n, x, s);
  const double2 *p = reinterpret_cast<const double2 *>(c + (size_t)i * istride);
  const double2 *q = reinterpret_cast<const double2 *>(c + (size_t)i * istride + ro);
  const double2 a01 = p[0], a23 = p[1], a45 = p[2], b01 = q[0], b23 = q[1], b45 = q[2];
  a = horner6(a01, a23, a45, s);
  b = horner6(b01, b23, b45, s);
  if (x != x) a = b = __builtin_nan("");
}
// ABI v4 rows on a function's own theta nodes (include/mpcekf.h node / node_p): the segment
// k = #{j in 1..m-2 : x_j <= theta} (oracle node_poly) from the function's uniform bucket map
// (host build_rom: nu buckets over [0, 1], nu a power of two, each bucket holding at most
// one interior node; entry u = (k of u / nu, x_k, x_k+1 or +inf)): floor(theta nu) is exact,
// so the bucket's left edge lies at or below theta and one compare with x_k+1 finishes the
// search.  s = theta - x_k, then Horner over the segment's 6 coefficients as tabp2.
__device__ __forceinline__ void tabn2(const double *c, const double *map, int nu, double x, int istride, double &a,
                                      double &b, int ro) {
  const double xc = fmin(fmax(x, 0.0), 1.0);  // NaN x: 0 (fmax), the NaN selected below
  int u = (int)floor(xc * (double)nu);
  u = u > nu - 1 ? nu - 1 : u;
  const double2 *m = reinterpret_cast<const double2 *>(map + (size_t)u * KMAP);
  const double2 m0 = m[0], m1 = m[1];
  const bool up = xc >= m1.x;
  const int i = (int)m0.x + (up ? 1 : 0);
  const double s = xc - (up ? m1.x : m0.y);
  const double2 *p = reinterpret_cast<const double2 *>(c + (size_t)i * istride);
  const double2 *q = reinterpret_cast<const double2 *>(c + (size_t)i * istride + ro);
  const double2 a01 = p[0], a23 = p[1], a45 = p[2], b01 = q[0], b23 = q[1], b45 = q[2];
  a = horner6(a01, a23, a45, s);
  b = horner6(b01, b23, b45, s);
  if (x != x) a = b = __builtin_nan("");
}
// Electrode tables (include/mpcekf.h mpcekf_electrode; host: build_rom).  In LDS: a
// header [Uocp1 [side][nth] | TK [MAXTT] | soc(0,T), soc(1,T) [side][2][MAXTT]], then
// the 2-D tables [EF_*][side][nte][nth].  EF_CDL is last and only the plant blob
// carries it (k_cell / k_bounds never read Cdleff).  A cell's temperature bracket
// (j, g) is found once per step (bracket); a lookup is then the theta interpolation of
// rows j and j + 1 and a + g (b - a), the sequence of oracle/mpcekf_oracle.c tab2/tidx.
// ABI v3 tables (KRom::npoly): the LDS header holds no Uocp1 and no 2-D tables follow
// but the lookup descriptors; the rows are polynomials in KRom::poly, and a function with
// Ea != 0 is multiplied by its Arrhenius factor dexp(Ea/R (1/Tref - 1/T)).
// permuted row q carries the (single-bit) flag G: bit q of that flag's row mask
__device__ __forceinline__ bool rowf(const KRom &r, int q, unsigned G) {
  return (r.fmask[__builtin_ctz(G)] >> q) & 1u;
}

enum { EF_U = 0, EF_DU, EF_K0, EF_RF, EF_CDL, NEF };
__host__ __device__ constexpr int etab_header(int nth) { return 2 * nth + 5 * MAXTT; }
// v3: the 12 lookup descriptors after the soc ends (d = fn * 2 + side, Uocp1 10 + side),
// KDESC doubles each: Ea/R, then int32 pairs (off, istride), (jstride, ro), (mapoff, nu) as
// raw bits (nu = 0: the uniform grid; v4: the function's bucket map at poly + mapoff)
__host__ __device__ constexpr int etab_desc(int hn) { return 2 * hn + 5 * MAXTT; }
struct ETab {
  const double *b;  // LDS base of the tables
  const KRom *r;    // v3: the polynomial table and the Arrhenius energies
  bool pl;          // v3 tables: a constant of the instantiation (etab<PL>), so each kernel
                    // compiles one lookup (the linear kernels are the round-4 code)
  int nth, nte;
  int hn;           // Uocp1 points in the LDS header: nth (v2), 0 (v3)
  int j;            // temperature bracket of this cell-step
  double g;
  double xa;        // v3: 1/Tref - 1/T of this cell-step (T unclamped)
  // v3 device layout (host build_rom): per function and electrode, interval-major with the
  // nte temperature rows of an interval adjacent, [fn][side][nth-1][nte][KPOLY], so the two
  // rows of a bracket are one 96-byte span; a T-invariant function (all rows equal, e.g. an
  // exact Arrhenius one) keeps one row, [nth-1][1][KPOLY]; Uocp1 last.  Where each function's
  // rows are and its Ea/R come from its descriptor in the LDS header (etab_desc): values in
  // VGPRs read at the lookup, so a kernel holds no per-function scalars (the 2 x 5 offsets
  // and energies as kernel arguments cost ~1,100 SGPR-spill reloads in k_cell).  One code
  // path: the rows of interval i at bracket j are at off + j jstride + i istride and + ro
  // (a T-invariant or single-temperature function: jstride = ro = 0, its row blended with
  // itself, a + g (a - a) = a, oracle tab2)
  __device__ __forceinline__ double f(int side, int fn, double th) const {
    if (pl) {
      const double *dp = b + etab_desc(hn) + (fn * 2 + side) * KDESC;
      const double ear = dp[0];
      const long long w0 = __double_as_longlong(dp[1]), w1 = __double_as_longlong(dp[2]);
      const int off = (int)w0, istr = (int)(w0 >> 32), jstr = (int)w1, ro = (int)(w1 >> 32);
      double a, c;
      int nu = 0, moff = 0;
      if (r->nodes) {  // a uniform flag: v3 ROMs never read the map word
        const long long w3 = __double_as_longlong(dp[3]);
        nu = __builtin_amdgcn_readfirstlane((int)(w3 >> 32));
        moff = __builtin_amdgcn_readfirstlane((int)w3);
      }
      if (nu == 0)
        tabp2(r->poly + off + j * jstr, nth, th, istr, a, c, ro);
      else
        tabn2(r->poly + off + j * jstr, r->poly + moff, nu, th, istr, a, c, ro);
      a = a + g * (c - a);
      // every function multiplied by its factor, dexp(+-0) = 1 exactly when Ea = 0 (a * 1 = a:
      // the oracle's unmultiplied value): no branch between neighbouring lookups' loads
      a = a * dexp(ear != 0.0 ? ear * xa : 0.0);
      return a;
    }
    const double *t = b + etab_header(nth) + ((fn * 2 + side) * nte + j) * nth;
    const double a = tabi(t, nth, th);
    if (nte == 1) return a;
    const double c = tabi(t + nth, nth, th);
    return a + g * (c - a);
  }
  __device__ __forceinline__ double u1(int side, double th) const {
    if (pl) {
      const double *dp = b + etab_desc(hn) + (10 + side) * KDESC;
      const long long w0 = __double_as_longlong(dp[1]);
      if (r->nodes) {
        const long long w3 = __double_as_longlong(dp[3]);
        const int nu = __builtin_amdgcn_readfirstlane((int)(w3 >> 32));
        if (nu) {
          double a, c;
          tabn2(r->poly + (int)w0, r->poly + __builtin_amdgcn_readfirstlane((int)w3), nu, th, (int)(w0 >> 32), a, c, 0);
          return a;
        }
      }
      return tabp(r->poly + (int)w0, nth, th, (int)(w0 >> 32));
    }
    return tabi(b + side * nth, nth, th);
  }
  __device__ __forceinline__ double tk(int i) const { return b[2 * hn + i]; }
  __device__ __forceinline__ double send(int side, int one) const {  // soc(one, T) at the bracket
    const double *t = b + 2 * hn + MAXTT + (side * 2 + one) * MAXTT;
    if (nte == 1) return t[0];
    return t[j] + g * (t[j + 1] - t[j]);
  }
  __device__ __forceinline__ void bracket(double T) {
    j = 0;
    g = 0.0;
    xa = pl && r->arr ? 1.0 / r->Tref - 1.0 / T : 0.0;
    if (nte == 1) return;
    const double Tc = fmin(fmax(T, tk(0)), tk(nte - 1));
    int k = 0;
    while (k < nte - 2 && Tc >= tk(k + 1)) ++k;
    j = k;
    g = (Tc - tk(k)) / (tk(k + 1) - tk(k));
  }
  // soc(z,T) = soc0 + z (soc100 - soc0) (iterEKF.m:282-283)
  __device__ __forceinline__ double soc(int side, double z) const {
    const double s0 = send(side, 0), s1 = send(side, 1);
    return s0 + z * (s1 - s0);
  }
};
template <bool PL>
__device__ __forceinline__ ETab etab(const KRom &r, const double *base, double T) {
  ETab e;
  e.b = base;
  e.r = &r;
  e.pl = PL;
  e.nth = r.nth;
  e.nte = r.nte;
  e.hn = PL ? 0 : r.nth;
  e.bracket(T);
  return e;
}

__device__ __forceinline__ void two_nearest(const double *pts, int n, double x, int &i1, int &i2) {
  int b1 = -1, b2 = -1;
  double d1 = 0.0, d2 = 0.0;
  for (int i = 0; i < n; ++i) {
    double d = fabs(x - pts[i]);
    bool better1 = b1 < 0 || (d < d1) || (d1 != d1 && d == d);
    if (better1) {
      b2 = b1; d2 = d1; b1 = i; d1 = d;
      continue;
    }
    bool better2 = b2 < 0 || (d < d2) || (d2 != d2 && d == d);
    if (better2) { b2 = i; d2 = d; }
  }
  i1 = b1;
  i2 = b2 < 0 ? b1 : b2;
}

struct XI {
  double g[4];
  int m[4];
};

// iterEKF.m:219-255
__device__ __forceinline__ void get_xind(int nT, int nZ, const double *Tp, const double *Zp, double Tk, double SOC,
                                         XI &xi) {
  int iZu = 0, iZl = 0, iTu = 0, iTl = 0;
  if (nZ > 1) {
    int a, b;
    two_nearest(Zp, nZ, SOC, a, b);
    iZu = a; iZl = b;
    if (Zp[iZu] < Zp[iZl]) { iZu = b; iZl = a; }
  }
  if (nT > 1) {
    int a, b;
    two_nearest(Tp, nT, Tk, a, b);
    iTu = a; iTl = b;
    if (Tp[iTu] < Tp[iTl]) { iTu = b; iTl = a; }
  }
  double aZ = 0.0, aT = 0.0;
  if (nZ > 1) aZ = (SOC - Zp[iZl]) / (Zp[iZu] - Zp[iZl]);
  if (nT > 1) aT = (Tk - Tp[iTl]) / (Tp[iTu] - Tp[iTl]);
  xi.g[0] = (1 - aT) * (1 - aZ);
  xi.g[1] = (1 - aT) * aZ;
  xi.g[2] = aT * (1 - aZ);
  xi.g[3] = aT * aZ;
  xi.m[0] = iTl * nZ + iZl;
  xi.m[1] = iTl * nZ + iZu;
  xi.m[2] = iTu * nZ + iZl;
  xi.m[3] = iTu * nZ + iZu;
}

// A corner record as REC / 2 pairs of doubles, pair e at rec2[e * st]: st = 1 is the record in
// s.ekf, st = n a slot of the corner window (KState::hot_rec).  The stride is a per-lane value
// where a lane takes its record from either place; the loads and stores are the same 16-byte
// ones in both.
__device__ __forceinline__ void load_x(const double *rec, double x[NX], size_t st = 1) {
  const double2 *p = reinterpret_cast<const double2 *>(rec);
  double2 a = p[0], b = p[st];
  x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  x[4] = reinterpret_cast<const double *>(p + 2 * st)[0];
}
__device__ __forceinline__ void load_rec(const double *rec, double x[NX], double S[NPK], size_t st = 1) {
  const double2 *p = reinterpret_cast<const double2 *>(rec);
  double v[REC];
#pragma unroll
  for (int i = 0; i < REC / 2; ++i) {
    double2 t = p[i * st];
    v[2 * i] = t.x;
    v[2 * i + 1] = t.y;
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = v[i];
#pragma unroll
  for (int i = 0; i < NPK; ++i) S[i] = v[NX + i];
}
__device__ __forceinline__ void store_rec(double *rec, const double x[NX], const double S[NPK], size_t st = 1) {
  double2 *p = reinterpret_cast<double2 *>(rec);
  double v[REC];
#pragma unroll
  for (int i = 0; i < NX; ++i) v[i] = x[i];
#pragma unroll
  for (int i = 0; i < NPK; ++i) v[NX + i] = S[i];
#pragma unroll
  for (int i = 0; i < REC / 2; ++i) p[i * st] = make_double2(v[2 * i], v[2 * i + 1]);
}
__device__ __forceinline__ void load_S(const double *rec, double S[NPK], size_t st = 1) {
  const double2 *p = reinterpret_cast<const double2 *>(rec);
  S[0] = reinterpret_cast<const double *>(p + 2 * st)[1];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    double2 t = p[(3 + i) * st];
    S[1 + 2 * i] = t.x;
    S[2 + 2 * i] = t.y;
  }
}
// slot j of cell c in the corner window, as a record pointer for the accessors above (st = n)
__device__ __forceinline__ double *hot_slot(const KState &s, int j, int64_t c) {
  return s.hot_rec + 2 * ((size_t)j * HOT_PAIRS * (size_t)s.n + (size_t)c);
}

// ---------------------------------------------------------------------------
// Cyclic Jacobi on a packed symmetric 5x5 (orc_jacobi), V row-major 5x5.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void jacobi5(double a[NPK], double V[NX * NX]) {
#pragma unroll
  for (int i = 0; i < NX * NX; ++i) V[i] = (i % (NX + 1)) == 0 ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      dg = dg + a[pk(p, p)] * a[pk(p, p)];
#pragma unroll
      for (int q = p + 1; q < NX; ++q) off = off + a[pk(p, q)] * a[pk(p, q)];
    }
    if (!(off > 1e-36 * dg)) break;
#pragma unroll
    for (int p = 0; p < NX - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < NX; ++q) {
        double apq = a[pk(p, q)];
        if (apq != 0.0) {
          double theta = (a[pk(q, q)] - a[pk(p, p)]) / (2.0 * apq);
          double t;
          if (fabs(theta) > 1e150) {
            t = 0.5 / theta;
          } else {
            t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0) t = -t;
          }
          double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
          a[pk(p, p)] = a[pk(p, p)] - t * apq;
          a[pk(q, q)] = a[pk(q, q)] + t * apq;
          a[pk(p, q)] = 0.0;
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            if (r == p || r == q) continue;
            double g = a[pk(r, p)], h = a[pk(r, q)];
            a[pk(r, p)] = g - s * (h + g * tau);
            a[pk(r, q)] = h + s * (g - h * tau);
          }
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            double g = V[r * NX + p], h = V[r * NX + q];
            V[r * NX + p] = g - s * (h + g * tau);
            V[r * NX + q] = h + s * (g - h * tau);
          }
        }
      }
    }
  }
}

// Positive definiteness of a packed symmetric 5x5 by LDL' pivots (orc_is_pd, same order).
// sc: a = sc * the given array (1.0: a itself), applied where an entry is read.
__device__ __forceinline__ bool is_pd5(const double a[NPK], double sc = 1.0) {
  double l[NX][NX], d[NX];
  bool pd = true;
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    double s = a[pk(j, j)] * sc;
#pragma unroll
    for (int k = 0; k < j; ++k) s = __builtin_fma(-(l[j][k] * l[j][k]), d[k], s);
    pd = pd && (s > 0);
    d[j] = s;
    if (j + 1 < NX) {
      const double inv = 1.0 / s;
#pragma unroll
      for (int i = j + 1; i < NX; ++i) {
        double t = a[pk(j, i)] * sc;
#pragma unroll
        for (int k = 0; k < j; ++k) t = __builtin_fma(-(l[i][k] * l[j][k]), d[k], t);
        l[i][j] = t * inv;
      }
    }
  }
  return pd;
}

// The symmetrisation of meas_update_regs when some lane of the wave is not positive
// definite: HH = V|Lambda|V' by Jacobi (out of line: rare, and its registers would
// otherwise weigh on every caller).
template <bool INL>
__device__ __forceinline__ void meas_polar(const double Ps[NPK], double a[NPK], double S[NPK], bool pd, bool bump) {
  double H[NPK];
#pragma unroll
  for (int i = 0; i < NPK; ++i) H[i] = a[i];
  double V[NX * NX];
  jacobi5(a, V);
  double w[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) w[k] = fabs(a[pk(k, k)]);
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = r; c < NX; ++c) {
      double hrc = 0.0, hcr = 0.0;
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        hrc = hrc + (V[r * NX + k] * w[k]) * V[c * NX + k];
        hcr = hcr + (V[c * NX + k] * w[k]) * V[r * NX + k];
      }
      if (pd) { hrc = H[pk(r, c)]; hcr = H[pk(r, c)]; }
      double v = ((Ps[pk(r, c)] + hrc) + hcr) / 4.0;
      if (bump) v = v * 2.0;
      S[pk(r, c)] = v;
    }
}

__device__ __noinline__ void meas_polar_slow(const double Ps[NPK], double a[NPK], double S[NPK], bool pd,
                                             bool bump) {
  meas_polar<false>(Ps, a, S, pd, bump);
}

// iterEKF.m:137-153 on one corner record (orc_meas_cov + state update).
// P = Sigma - (L*St)*L' is only ever used as P + P', so only that sum is kept.
template <bool OUTLINE = false>  // OUTLINE: the Jacobi branch as a call (k_ekf4's 128/256-VGPR budget)
__device__ __forceinline__ void meas_update_regs(double x[NX], double S[NPK], const double L[NX], double St,
                                                 double res) {
#pragma unroll
  for (int k = 0; k < NX; ++k) x[k] = __builtin_fma(L[k], res, x[k]);
  double LS[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) LS[r] = L[r] * St;
  double Ps[NPK];
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = r; c < NX; ++c) {
      double prc = __builtin_fma(-LS[r], L[c], S[pk(r, c)]);
      double pcr = __builtin_fma(-LS[c], L[r], S[pk(r, c)]);
      Ps[pk(r, c)] = prc + pcr;
    }
  // a = (P + P')/2 = Ps * 0.5: the same operation on the same sum, formed where it is
  // used (not held: an array of 15 doubles less at the kernel's register peak)
  const bool bump = res * res > 9 * St;
  // HH = VV*SS*VV' (iterEKF.m:145-146) is the polar factor of the symmetric part a:
  // a itself when a is positive definite (the usual case), else V|Lambda|V' (Jacobi).
  // The decomposition runs only if some lane of the wave needs it.
  const bool pd = is_pd5(Ps, 0.5);
  if (__all(pd)) {
#pragma unroll
    for (int i = 0; i < NPK; ++i) {
      const double a = Ps[i] * 0.5;
      double v = ((Ps[i] + a) + a) / 4.0;
      if (bump) v = v * 2.0;
      S[i] = v;
    }
  } else {
    double a[NPK];
#pragma unroll
    for (int i = 0; i < NPK; ++i) a[i] = Ps[i] * 0.5;
    if constexpr (OUTLINE) meas_polar_slow(Ps, a, S, pd, bump);
    else meas_polar<true>(Ps, a, S, pd, bump);
  }
}

__device__ __forceinline__ void meas_update(double *rec, const double L[NX], double St, double res) {
  double x[NX], S[NPK];
  load_rec(rec, x, S);
  meas_update_regs(x, S, L, St, res);
  store_rec(rec, x, S);
}

// ---------------------------------------------------------------------------
// Per-lane context for one cell
// ---------------------------------------------------------------------------
struct CellCtx {
  const double *L;   // LDS: model blob base
  const double *Tp, *Zp;  // LDS set-points
  double *erec;      // this cell's EKF records in HBM
  int stride;
  double T;          // iterEKF's Tk in K (iterEKF.m:62-66)
  ETab et;           // electrode tables, bracketed at T
};

// getVariables (iterEKF.m:259-417).  Z is the permuted output vector.
// QUAD: a lane quad per cell (k_ekf4): this lane's corner is qj with state xr[0]; the
// corner sums Z = fma(z_j, g_j, Z), j = 0..3 in order, take z_j from lane j by DPP.
// k0 and Rf of one getVariables call at its SOCnAvg / SOCpAvg (after its clamps): getChatV
// (the same x0), getChatZ's scalars and EKFmatsHandler (the same x0 after the update) read
// k0 / Rf at the unclamped averages, which are these whenever no clamp fired -- the same
// lookup, so the same bits; they reuse the values then (fewer table reads, notably of
// the v3 polynomials) and look up otherwise
struct KR {
  double T, thn, thp, k0n, k0p, rfn, rfp;  // T: the lookups' temperature (EKFmatsHandler brackets its own)
};
__device__ __forceinline__ bool kr_hit(const KR *kr, double T, double thn, double thp) {
  return kr && kr->T == T && kr->thn == thn && kr->thp == thp;
}
template <int NZ, bool QUAD = false>
__device__ __forceinline__ double get_vars(const KRom &r, const CellCtx &cc, const XI &xi, double ik, double x0,
                                           double SOC0, int &warn, int &st, double Z[NZ], double &Zsoc,
                                           const double (*xr)[NX] = nullptr, int qj = 0, KR *kr = nullptr) {
  double xSOC = SOC0 - x0 * (r.Ts / (3600 * r.Q));
  double SOCnAvg = cc.et.soc(0, xSOC);
  double SOCpAvg = cc.et.soc(1, xSOC);
  if (SOCnAvg < 0) { warn++; SOCnAvg = 1e-6; }
  if (SOCnAvg > 1) { warn++; SOCnAvg = 1 - 1e-6; }
  if (SOCpAvg < 0) { warn++; SOCpAvg = 1e-6; }
  if (SOCpAvg > 0.998) { warn++; SOCpAvg = 0.998; }
#pragma unroll
  for (int q = 0; q < NZ; ++q) Z[q] = 0.0;
  if constexpr (QUAD) {
    const double *Cm = cc.L + xi.m[qj] * cc.stride;
    const double *Dm = Cm + NZ * NX;
    double cr[NX + 1];
#pragma unroll
    for (int k = 0; k < NX; ++k) cr[k] = Cm[k];
    cr[NX] = Dm[0];
#pragma unroll
    for (int q = 0; q < NZ; ++q) {
      double cn[NX + 1];
      if (q + 1 < NZ) {
#pragma unroll
        for (int k = 0; k < NX; ++k) cn[k] = Cm[(q + 1) * NX + k];
        cn[NX] = Dm[q + 1];
      }
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NX; ++k) acc = __builtin_fma(cr[k], xr[0][k], acc);
      const double zj = __builtin_fma(cr[NX], ik, acc);
      double zz = __builtin_fma(qbc<0>(zj), xi.g[0], 0.0);
      zz = __builtin_fma(qbc<1>(zj), xi.g[1], zz);
      zz = __builtin_fma(qbc<2>(zj), xi.g[2], zz);
      Z[q] = __builtin_fma(qbc<3>(zj), xi.g[3], zz);
      launder(Z[q]);  // rows in order: the next row's operands are the only ones in flight
      if (q + 1 < NZ) {
#pragma unroll
        for (int k = 0; k <= NX; ++k) cr[k] = cn[k];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < (QUAD ? 0 : 4); ++j) {
    double x[NX];
    if (xr) {
#pragma unroll
      for (int k = 0; k < NX; ++k) x[k] = xr[j][k];
    } else {
      load_x(cc.erec + (size_t)xi.m[j] * REC, x);
    }
    const double *Cm = cc.L + xi.m[j] * cc.stride;
    const double *Dm = Cm + NZ * NX;
    double g = xi.g[j];
    // row q+1's C and D are read while row q computes (LDS latency off the chain)
    double cr[NX + 1];
#pragma unroll
    for (int k = 0; k < NX; ++k) cr[k] = Cm[k];
    cr[NX] = Dm[0];
#pragma unroll
    for (int q = 0; q < NZ; ++q) {
      double cn[NX + 1];
      if (q + 1 < NZ) {
#pragma unroll
        for (int k = 0; k < NX; ++k) cn[k] = Cm[(q + 1) * NX + k];
        cn[NX] = Dm[q + 1];
      }
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NX; ++k) acc = __builtin_fma(cr[k], x[k], acc);
      const double zj = __builtin_fma(cr[NX], ik, acc);
      Z[q] = __builtin_fma(zj, g, Z[q]);
      launder(Z[q]);
      if (q + 1 < NZ) {
#pragma unroll
        for (int k = 0; k <= NX; ++k) cr[k] = cn[k];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_sched_barrier(0);
  double If0 = Z[R_IF0], If3 = Z[R_IF3];
  bool any = false;
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_NTH)) { Z[q] = Z[q] + SOCnAvg; any |= Z[q] < 0; }
  if (any) {
    warn++;
#pragma unroll
    for (int q = 0; q < NZ; ++q)
      if ((rowf(r, q, G_NTH)) && Z[q] < 0) Z[q] = 1e-6;
  }
  any = false;
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_NTH)) any |= Z[q] > 1;
  if (any) {
    warn++;
#pragma unroll
    for (int q = 0; q < NZ; ++q)
      if ((rowf(r, q, G_NTH)) && Z[q] > 1) Z[q] = 1 - 1e-6;
  }
  any = false;
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_PTH)) { Z[q] = Z[q] + SOCpAvg; any |= Z[q] < 0; }
  if (any) {
    warn++;
#pragma unroll
    for (int q = 0; q < NZ; ++q)
      if ((rowf(r, q, G_PTH)) && Z[q] < 0) Z[q] = 1e-6;
  }
  any = false;
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_PTH)) any |= Z[q] > 0.998;
  if (any) {
    warn++;
#pragma unroll
    for (int q = 0; q < NZ; ++q)
      if ((rowf(r, q, G_PTH)) && Z[q] > 0.998) Z[q] = 0.998;
  }
  double Un = cc.et.f(0, EF_U, SOCnAvg), Up = cc.et.f(1, EF_U, SOCpAvg);
#pragma unroll
  for (int q = 0; q < NZ; ++q) {
    if (rowf(r, q, G_NPHISE)) Z[q] = Z[q] + Un;
    if (rowf(r, q, G_PPHISE)) Z[q] = Z[q] + Up;
  }
  double PhieTilde3 = Z[R_PHIE];
  double Phise0 = Z[R_PHISE0];
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_PHIE)) {
      if (rowf(r, q, G_PHIE0)) Z[q] = 0 - Phise0;
      else Z[q] = Z[q] - Phise0;
    }
  any = false;
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_THETAE)) { Z[q] = Z[q] + 1; any |= Z[q] < 0; }
  if (any) {  // iterEKF.m:384-389 would raise a MATLAB error
    warn++;
    st |= ST_ERROR | ST_THETAE_NEG;
    return __builtin_nan("");
  }
  double k0n = cc.et.f(0, EF_K0, SOCnAvg), k0p = cc.et.f(1, EF_K0, SOCpAvg);  // iterEKF.m:392-393
  double i0n = k0n * sqrt(Z[R_TE1] * (1 - Z[R_TH0]) * Z[R_TH0]);
  double i0p = k0p * sqrt(Z[R_TEE] * (1 - Z[R_TH3]) * Z[R_TH3]);
  double negEta0 = 2 * r.R * cc.T / r.F * dasinh(If0 / (2 * i0n));
  double posEta3 = 2 * r.R * cc.T / r.F * dasinh(If3 / (2 * i0p));
  double Uocpn0 = cc.et.f(0, EF_U, Z[R_TH0]), Uocpp3 = cc.et.f(1, EF_U, Z[R_TH3]);
  double Rfn = cc.et.f(0, EF_RF, SOCnAvg), Rfp = cc.et.f(1, EF_RF, SOCpAvg);  // iterEKF.m:406-407
  if (kr) *kr = KR{cc.T, SOCnAvg, SOCpAvg, k0n, k0p, Rfn, Rfp};
  double V = posEta3 - negEta0 + PhieTilde3 + Uocpp3 - Uocpn0 + (Rfp * Z[R_IFDL3] - Rfn * Z[R_IFDL0]);
#pragma unroll
  for (int q = 0; q < NZ; ++q)
    if (rowf(r, q, G_PPHIS)) Z[q] = Z[q] + V;
  Zsoc = SOC0 - x0 * (r.Ts / (3600 * r.Q));
  return V;
}

// getChatV (iterEKF.m:421-519) pieces.  Cell scalars of the voltage Jacobian.
struct ChatK {
  double Rfn, Rfp, Rctn, Rctp, dUn0, dUp3, dn, dp;
};
// xSOC = SOC0 - x0 Ts/(3600 Q) with the x0 of the call: Rf and k0 at the unclamped
// soc(xSOC, Tk) (iterEKF.m:437-442,463-464)
__device__ __forceinline__ ChatK chat_k(const KRom &r, const CellCtx &cc, double xSOC, double zTE1, double zTH0,
                                        double zTEE, double zTH3, const KR *kr = nullptr) {
  ChatK k;
  const double SOCnAvg = cc.et.soc(0, xSOC), SOCpAvg = cc.et.soc(1, xSOC);
  double k0n, k0p;
  if (kr_hit(kr, cc.T, SOCnAvg, SOCpAvg)) {
    k.Rfn = kr->rfn;
    k.Rfp = kr->rfp;
    k0n = kr->k0n;
    k0p = kr->k0p;
  } else {
    k.Rfn = cc.et.f(0, EF_RF, SOCnAvg);
    k.Rfp = cc.et.f(1, EF_RF, SOCpAvg);
    k0n = cc.et.f(0, EF_K0, SOCnAvg);
    k0p = cc.et.f(1, EF_K0, SOCpAvg);
  }
  double i0n = k0n * sqrt(zTE1 * (1 - zTH0) * zTH0);
  double i0p = k0p * sqrt(zTEE * (1 - zTH3) * zTH3);
  k.Rctn = r.R * cc.T / (r.F * i0n);
  k.Rctp = r.R * cc.T / (r.F * i0p);
  k.dUn0 = cc.et.f(0, EF_DU, zTH0);
  k.dUp3 = cc.et.f(1, EF_DU, zTH3);
  k.dn = cc.et.soc(0, 1) - cc.et.soc(0, 0);  // soc(1,Tk) - soc(0,Tk) (iterEKF.m:497-500)
  k.dp = cc.et.soc(1, 1) - cc.et.soc(1, 0);
  return k;
}
// The row of one corner (model blob Cm, interpolation weight g).
__device__ __forceinline__ void chat_row(const KRom &r, const ChatK &K, const double *Cm, double g, double Chat[NX]) {
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    double v = K.Rfp * (g * Cm[R_IFDL3 * NX + k]) - K.Rfn * (g * Cm[R_IFDL0 * NX + k]);
    v = v + K.Rctp * (g * Cm[R_IF3 * NX + k]) - K.Rctn * (g * Cm[R_IF0 * NX + k]);
    v = v + g * Cm[R_PHIE * NX + k];
    v = v + (K.dUp3 * (g * Cm[R_TH3 * NX + k]) - K.dUn0 * (g * Cm[R_TH0 * NX + k]));
    Chat[k] = v;
  }
}
__device__ __forceinline__ double chat0(const KRom &r, const ChatK &K) {
  double res0n = -K.dUn0 * r.Ts * K.dn / (3600 * r.Q);
  double res0p = -K.dUp3 * r.Ts * K.dp / (3600 * r.Q);
  return res0p - res0n;
}
// Voltage Jacobian rows of the 4 corners.
template <int NZ>
__device__ __forceinline__ void get_chatv(const KRom &r, const CellCtx &cc, const XI &xi, double xSOC, double zTE1,
                                          double zTH0, double zTEE, double zTH3, double Chat[4][NX], double &Chat0,
                                          const KR *kr = nullptr) {
  const ChatK K = chat_k(r, cc, xSOC, zTE1, zTH0, zTEE, zTH3, kr);
#pragma unroll
  for (int j = 0; j < 4; ++j) chat_row(r, K, cc.L + xi.m[j] * cc.stride, xi.g[j], Chat[j]);
  Chat0 = chat0(r, K);
}

// getChatZ's scalars at the updated state (iterEKF.m:190, 543, 562-580): for k_bounds
struct BoundK {
  ChatK K;
  double C0, r0n, r0p, dUn, dUp;
};
__device__ __forceinline__ BoundK bound_k(const KRom &r, const CellCtx &cc, double xSOC, double zTE1, double zTH0,
                                          double zTEE, double zTH3, const KR *kr = nullptr) {
  BoundK b;
  b.K = chat_k(r, cc, xSOC, zTE1, zTH0, zTEE, zTH3, kr);
  b.C0 = chat0(r, b.K);
  b.r0n = -r.Ts * b.K.dn / (3600 * r.Q);  // iterEKF.m:562-565
  b.r0p = -r.Ts * b.K.dp / (3600 * r.Q);
  b.dUn = cc.et.f(0, EF_DU, cc.et.soc(0, xSOC));  // iterEKF.m:576-580
  b.dUp = cc.et.f(1, EF_DU, cc.et.soc(1, xSOC));
  return b;
}
__device__ __forceinline__ double bound_field(const BoundK &b, int i) {  // BD_K + i, i < 11
  switch (i) {
    case 0: return b.K.Rfn;
    case 1: return b.K.Rfp;
    case 2: return b.K.Rctn;
    case 3: return b.K.Rctp;
    case 4: return b.K.dUn0;
    case 5: return b.K.dUp3;
    case 6: return b.C0;
    case 7: return b.r0n;
    case 8: return b.r0p;
    case 9: return b.dUn;
    default: return b.dUp;
  }
}

// MPC pieces (predMat.m, constraintsMPC.m, iterMPC.m) live in mpcekf_mpc.hpp,
// templated on the horizons; this file instantiates them for NP x NC.

// EKFmatsHandler.m:26-114.  zTE1.. are the role rows of zk, Zsoc = zk(end).
// EKFmatsHandler.m:26-31: the corner of largest weight, first of equals; max()
// skips NaN weights.
// The running maximum and its model index are carried in registers: xi.g[imax] / xi.m[imax]
// with a run-time imax would keep the whole XI in scratch.
__device__ __forceinline__ int corner_max(const XI &xi, int *mmax = nullptr) {
  int imax = 0, m = xi.m[0];
  double gm = xi.g[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const double gj = xi.g[j];
    int mj = xi.m[j];
    asm("" : "+v"(mj));  // a value: a select of two loads would be folded into one indexed load
    if (gj > gm || (gm != gm && gj == gj)) {
      imax = j;
      gm = gj;
      m = mj;
    }
  }
  if (mmax) *mmax = m;
  return imax;
}

// xm (use_xm): that corner's xhat when the caller holds it in registers (k_cell's fused
// step), else read from its record
template <int NZ>
__device__ __forceinline__ void mats_handler(const KRom &r, const CellCtx &cc, const XI &xi, const double *zr,
                                             double Zsoc, double TK, Lin &L, double xend, const double (&xm)[NX],
                                             bool use_xm, const KR *kr = nullptr) {
  int m;
  (void)corner_max(xi, &m);
  const double *Cm = cc.L + m * cc.stride;
  const double *Dm = Cm + NZ * NX;
  const double *am = Dm + NZ;
  double x[NX];
  if (use_xm) {
#pragma unroll
    for (int k = 0; k < NX; ++k) x[k] = xm[k];
  } else {
    load_x(cc.erec + (size_t)m * REC, x);
  }
#pragma unroll
  for (int k = 0; k < NX; ++k) { L.xhat[k] = x[k]; L.a[k] = am[k]; }
  L.xhat[NX] = xend;  // ekfData.xhat(end) (EKFmatsHandler.m:33): 0 in 'OB', the MB integrator
  L.a[NX] = 1.0;
  double rr = -r.Ts / (3600 * r.Q);
#pragma unroll
  for (int k = 0; k < 6; ++k) L.Csoc[k] = 0.0;
  L.Csoc[NX] = rr;
  L.Dsoc = 0.0;
  ETab et = cc.et;
  et.bracket(TK);  // EKFmatsHandler.m:53: TK = Tk + 273.15
  double SOCnAvg = et.soc(0, Zsoc), SOCpAvg = et.soc(1, Zsoc);  // EKFmatsHandler.m:57-58
  double k0n, k0p, Rfn, Rfp;  // EKFmatsHandler.m:60-61,68-69 (the second getVariables' when its averages)
  if (kr_hit(kr, TK, SOCnAvg, SOCpAvg)) {
    k0n = kr->k0n;
    k0p = kr->k0p;
    Rfn = kr->rfn;
    Rfp = kr->rfp;
  } else {
    k0n = et.f(0, EF_K0, SOCnAvg);
    k0p = et.f(1, EF_K0, SOCpAvg);
    Rfn = et.f(0, EF_RF, SOCnAvg);
    Rfp = et.f(1, EF_RF, SOCpAvg);
  }
  double i0n = k0n * sqrt(zr[R_TE1] * (1 - zr[R_TH0]) * zr[R_TH0]);
  double i0p = k0p * sqrt(zr[R_TEE] * (1 - zr[R_TH3]) * zr[R_TH3]);
#pragma unroll
  for (int k = 0; k < NX; ++k)
    L.Cv[k] = Rfp * Cm[R_IFDL3 * NX + k] - Rfn * Cm[R_IFDL0 * NX + k] + Cm[R_PHIE * NX + k];
  L.Cv[NX] = 0.0;
  L.Dv = Rfp * Dm[R_IFDL3] - Rfn * Dm[R_IFDL0] + Dm[R_PHIE];
  double Upos = et.f(1, EF_U, zr[R_TH3]), Uneg = et.f(0, EF_U, zr[R_TH0]);
  double negEta0 = 2 * r.R * TK / r.F * dasinh(zr[R_IF0] / (2 * i0n));
  double posEta3 = 2 * r.R * TK / r.F * dasinh(zr[R_IF3] / (2 * i0p));
  double b_phi = 0.01 * 0;
  L.bv = (Upos - Uneg) + (posEta3 - negEta0) + b_phi;
  L.bphi = et.u1(0, SOCnAvg);  // one-argument Uocp (EKFmatsHandler.m:96)
#pragma unroll
  for (int k = 0; k < NX; ++k) L.Cphi[k] = Cm[R_NPHISE2 * NX + k];
  L.Cphi[NX] = 0.0;
  L.Dphi = Dm[R_NPHISE2];
}

// hildreth.m:17-46.  H = M*(E\M') is re-formed entry by entry in the exact
// summation order of the dense product (orc_hildreth), never stored.
template <class MV>
__device__ __forceinline__ int hildreth_core(const MV &Mf, const double E[NC][NC], const double F[NC],
                                             const double gam[NCON], double lam[NCON], int maxIter, double tol,
                                             double DU[NC]) {
  double R[NC][NC];
  bool ok = chol_n<NC>(E, R);
  double X[NCON][NC];
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    double b[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) b[k] = Mf(i, k);
    mldiv_spd<NC>(E, R, ok, b, X[i]);
  }
  double y[NC];
  mldiv_spd<NC>(E, R, ok, F, y);
  double K[NCON];
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) s = s + Mf(i, k) * y[k];
    K[i] = s + gam[i];
  }
  bool fin = true;
#pragma unroll
  for (int i = 0; i < NCON; ++i)
#pragma unroll
    for (int k = 0; k < NC; ++k) fin = fin && isfinite(X[i][k]) && isfinite(Mf(i, k));
  // orc_hildreth's defined evaluation: rank-Nc form with v = X*lambda when X and M are
  // finite, else the dense H(i,:)*lambda as 4 interleaved partial sums
  auto xv = [&](double v[NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < NCON; ++j) a = __builtin_fma(X[j][k], lam[j], a);
      v[k] = a;
    }
  };
  int it;
  for (it = 1; it <= maxIter; ++it) {
#pragma unroll
    for (int i = 0; i < NCON; ++i)
#pragma unroll
      for (int k = 0; k < NC; ++k) launder(X[i][k]);
    bool conv = true;
    double v[NC];
    if (fin) xv(v);
#pragma unroll
    for (int i = 0; i < NCON; ++i) {
      double hii = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) hii = hii + Mf(i, k) * X[i][k];
      double s = 0.0, nl, d;
      if (fin) {
        double t = K[i];
#pragma unroll
        for (int k = 0; k < NC; ++k) t = __builtin_fma(Mf(i, k), v[k], t);
        d = hild_step(t, hii, 1.0 / hii, lam[i], nl);
      } else {
        double p4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < NCON; ++j) {
          double h = 0.0;
#pragma unroll
          for (int k = 0; k < NC; ++k) h = h + Mf(i, k) * X[j][k];
          p4[j & 3] = p4[j & 3] + h * lam[j];
        }
        s = (p4[0] + p4[1]) + (p4[2] + p4[3]);
        const double w = -((K[i] + s) - hii * lam[i]) / hii;
        nl = w > 0 ? w : 0.0;
        d = nl - lam[i];
      }
      if (!(fabs(d) < tol)) conv = false;
      lam[i] = nl;
      if (fin) {
        if (isfinite(d)) {
#pragma unroll
          for (int k = 0; k < NC; ++k) v[k] = __builtin_fma(X[i][k], d, v[k]);
        } else {
          xv(v);
        }
      }
    }
    if (conv) break;
  }
  if (it > maxIter) it = maxIter;
  double rhs[NC], mE[NC][NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NCON; ++i) s = s + Mf(i, k) * lam[i];
    rhs[k] = F[k] + s;
  }
#pragma unroll
  for (int a = 0; a < NC; ++a)
#pragma unroll
    for (int b = 0; b < NC; ++b) mE[a][b] = -E[a][b];
  lu_solve_n<NC>(mE, rhs, DU);
  return it;
}

// ---------------------------------------------------------------------------
// LDS staging
// ---------------------------------------------------------------------------
// The block's copy of a ROM blob (L2-resident, 30-130 KB) into LDS: 16 loads of 16 B per
// lane in flight before their stores.  A plain copy loop waited one L2 round trip per
// 16 B per lane (load, s_waitcnt vmcnt(0), ds_write): ~32 round trips for the cell blob.
__device__ __forceinline__ void stage_lds(double *dst, const double *src, int len) {
  constexpr int B = 16;
  const int n2 = len / 2, nt = blockDim.x;
  const double2 *s2 = reinterpret_cast<const double2 *>(src);
  double2 *d2 = reinterpret_cast<double2 *>(dst);
  int i = threadIdx.x;
  for (; i + (B - 1) * nt < n2; i += B * nt) {
    double2 v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) v[b] = s2[i + b * nt];
#pragma unroll
    for (int b = 0; b < B; ++b) d2[i + b * nt] = v[b];
  }
  // The remainder: clamped loads AND clamped stores, no branch.  With guarded stores the
  // compiler sank each load into its store's branch, so the remainder (up to 15 chunks per
  // lane for the cell blob) waited one L2 round trip per chunk.  Lanes past the end store
  // the last chunk's own value to the last chunk: the same bytes, whichever lane lands.
  if (n2 > 0) {
    double2 v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) v[b] = s2[min(i + b * nt, n2 - 1)];
#pragma unroll
    for (int b = 0; b < B; ++b) d2[min(i + b * nt, n2 - 1)] = v[b];
  }
  if ((len & 1) && threadIdx.x == 0) dst[len - 1] = src[len - 1];
}

// The ring inputs of a replay are loaded RCH steps at a time, all in flight together:
// a model first touched after a set-point crossing has up to LAZY_H - 1 skipped steps,
// and a load per step inside the loop waited one memory round trip each.  The FMAs then
// run in step order, so the bits are the per-step loop's.
#ifndef MPCEKF_RING_CHUNK
#define MPCEKF_RING_CHUNK 8
#endif
constexpr int RCH = MPCEKF_RING_CHUNK;
// ring[k % LAZY_H] for k = k0 .. k0 + RCH - 1 (clamped to kmax: a valid slot)
__device__ __forceinline__ void ring_chunk(const double *ring, const KState &s, int64_t c, int k0, int kmax,
                                           double v[RCH]) {
#pragma unroll
  for (int i = 0; i < RCH; ++i) v[i] = ring[(size_t)(min(k0 + i, kmax) % LAZY_H) * s.n + c];
}
// ---------------------------------------------------------------------------
// OB_step's simStep (OB_step.m:188-357), written once for every kernel that runs it:
// k_plant4, k_plant_obs, k_obs_traj, cell_plant (k_cell) and quad_plant (k_ekf4).  The routes
// agree bit for bit because they evaluate these expressions, in this order; where a call
// sits in a kernel's instruction stream, and its sched_barriers, are the kernel's own.
// ---------------------------------------------------------------------------
struct PlantCorners {
  int iZu, iZl, iTu, iTl;
};
// the two nearest SOC and temperature set points (0 on a single-set-point axis)
__device__ __forceinline__ PlantCorners plant_corners(const KRom &r, const double *Tp, const double *Zp,
                                                      double cellSOC, double T) {
  int iZu = 0, iZl = 0, iTu = 0, iTl = 0;
  if (r.nZ > 1) {
    int a, b;
    two_nearest(Zp, r.nZ, cellSOC, a, b);
    iZu = a > b ? a : b; iZl = a < b ? a : b;
  }
  if (r.nT > 1) {
    int a, b;
    two_nearest(Tp, r.nT, T, a, b);
    iTu = a > b ? a : b; iTl = a < b ? a : b;
  }
  return {iZu, iZl, iTu, iTl};
}
// corner j's model: mm = {Tl Zl, Tl Zu, Tu Zl, Tu Zu}[j] (OB_step.m:251-275)
__device__ __forceinline__ int corner_model(const KRom &r, const PlantCorners &pc, int j) {
  return ((j & 2) ? pc.iTu : pc.iTl) * r.nZ + ((j & 1) ? pc.iZu : pc.iZl);
}
__device__ __forceinline__ void corner_models(const KRom &r, const PlantCorners &pc, int mm[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) mm[j] = corner_model(r, pc, j);
}
// the blend weights of OB_step.m:285 (0 between duplicate corners)
__device__ __forceinline__ void plant_weights(const double *Tp, const double *Zp, const PlantCorners &pc,
                                              double cellSOC, double T, double &aZ, double &aT) {
  const double Zu = Zp[pc.iZu], Zl = Zp[pc.iZl], Tu = Tp[pc.iTu], Tl = Tp[pc.iTl];
  aZ = 0.0;
  aT = 0.0;
  if (Zu != Zl) aZ = (cellSOC - Zl) / (Zu - Zl);
  if (Tu != Tl) aT = (T - Tl) / (Tu - Tl);
}
// a corner's 6 states as three pairs, pair e at bx2[e * st]: st = 1 is the 48 B of bigx, st = n
// a slot of the plant window (KState::hotp_x); the same 16-byte loads and stores in both
__device__ __forceinline__ void load_corner(const double *bx, double xs[6], size_t st = 1) {
  const double2 *p = reinterpret_cast<const double2 *>(bx);
  const double2 q0 = p[0], q1 = p[st], q2 = p[2 * st];
  xs[0] = q0.x; xs[1] = q0.y; xs[2] = q1.x; xs[3] = q1.y; xs[4] = q2.x; xs[5] = q2.y;
}
__device__ __forceinline__ void store_corner(double *bx, const double x[6], size_t st = 1) {
  double2 *p = reinterpret_cast<double2 *>(bx);
  p[0] = make_double2(x[0], x[1]);
  p[st] = make_double2(x[2], x[3]);
  p[2 * st] = make_double2(x[4], x[5]);
}
// slot j of cell c in the plant window, as a state pointer for the two above (st = n)
__device__ __forceinline__ double *hotp_slot(const KState &s, int j, int64_t c) {
  return s.hotp_x + 2 * ((size_t)j * HOTP_PAIRS * (size_t)s.n + (size_t)c);
}
// the plant-window slot that holds model m of cell c (-1: none, its state is in bigx)
__device__ __forceinline__ int hotp_find(const KState &s, int64_t c, int m) {
  int slot = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (s.hotp_m[(size_t)i * s.n + c] == m) slot = i;
  return slot;
}
// SOCnAvg / SOCpAvg through this step (OB_step.m:212-219)
__device__ __forceinline__ void plant_soc_step(const KRom &r, const ETab &et, double SOC0n, double SOC0p, double Iapp,
                                               double &SOCnAvg, double &SOCpAvg) {
  const double Cdleffn = et.f(0, EF_CDL, SOC0n), Cdleffp = et.f(1, EF_CDL, SOC0p);
  double dUn = et.f(0, EF_DU, SOCnAvg), dUp = et.f(1, EF_DU, SOCpAvg);
  double dQn = fabs(r.th100n - r.th0n), dQp = fabs(r.th100p - r.th0p);
  double res0n = -dQn / (3600 * r.Q - Cdleffn * dQn * dUn);
  double res0p = dQp / (3600 * r.Q - Cdleffp * dQp * dUp);
  SOCnAvg = SOCnAvg + res0n * Iapp * r.Ts;
  SOCpAvg = SOCpAvg + res0p * Iapp * r.Ts;
  if (SOCnAvg < 0) SOCnAvg = 0;
  if (SOCnAvg > 1) SOCnAvg = 1;
  if (SOCpAvg < 0) SOCpAvg = 0;
  if (SOCpAvg > 1) SOCpAvg = 1;
}
// x = a .* xs + u (OB_step.m:198-200, 278; x may be xs).  A5: the integrator's a[5] = 1 is read
// from the blob (the plant and obs blobs carry it as data); otherwise a has NX entries and
// the 1 is a literal (the cell blob, checked by build_rom).
template <bool A5>
__device__ __forceinline__ void plant_advance(const double *a, const double xs[6], double u, double x[6]) {
#pragma unroll
  for (int e = 0; e < NX; ++e) x[e] = __builtin_fma(a[e], xs[e], u);
  x[NX] = __builtin_fma(A5 ? a[NX] : 1.0, xs[NX], u);
}
// the skipped steps tsj + 1 .. lazy_t - 1 of a corner, RCH ring inputs per round trip
template <bool A5>
__device__ __forceinline__ void plant_replay(double xs[6], const double *a, const KState &s, int64_t c, int tsj,
                                             int lazy_t) {
  for (int k0 = tsj + 1; k0 < lazy_t; k0 += RCH) {
    double u[RCH];
    ring_chunk(s.hist_u, s, c, k0, lazy_t - 1, u);
#pragma unroll
    for (int i = 0; i < RCH; ++i)
      if (k0 + i < lazy_t) plant_advance<A5>(a, xs, u[i], xs);
  }
}
// one output row of a corner, C x + res0 x5 + D Iapp summed from +0.0 (OB_step.m:251-275)
__device__ __forceinline__ double plant_row(const double *C, double r0, double d, const double xs[6], double Iapp) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < NX; ++k) acc = acc + C[k] * xs[k];
  acc = acc + r0 * xs[5];
  return acc + d * Iapp;
}
// the same row from the obs blob's [C 5][res0][D][0] record
__device__ __forceinline__ double obs_row(const double *B, const double xs[6], double Iapp) {
  const double2 *p = reinterpret_cast<const double2 *>(B);
  const double2 c01 = p[0], c23 = p[1], c4r = p[2], d = p[3];
  double acc = 0.0;
  acc = acc + c01.x * xs[0];
  acc = acc + c01.y * xs[1];
  acc = acc + c23.x * xs[2];
  acc = acc + c23.y * xs[3];
  acc = acc + c4r.x * xs[4];
  acc = acc + c4r.y * xs[5];
  return acc + d.x * Iapp;
}
// the four corners' rows blended (OB_step.m:285); quad_blend: lane j of a quad holds corner j's
__device__ __forceinline__ double blend4(double y0, double y1, double y2, double y3, double aZ, double aT) {
  return (1 - aT) * ((1 - aZ) * y0 + aZ * y1) + aT * ((1 - aZ) * y2 + aZ * y3);
}
__device__ __forceinline__ double quad_blend(double y, double aZ, double aT) {
  return blend4(qbc<0>(y), qbc<1>(y), qbc<2>(y), qbc<3>(y), aZ, aT);
}
// Vcell from the blended role rows (OB_step.m:329-356); reads yk only at the R_* indices
__device__ __forceinline__ double plant_vcell(const KRom &r, const ETab &et, const double *yk, double T, double Iapp,
                                              double negSOC, double posSOC, double SOC0n, double SOC0p) {
  double th0 = fmin(fmax(yk[R_TH0] + SOC0n, 1e-6), 1 - 1e-6);
  double th3 = fmin(fmax(yk[R_TH3] + SOC0p, 1e-6), 1 - 1e-6);
  double te1 = fmax(yk[R_TE1] + 1, 1e-6);
  double teE = fmax(yk[R_TEE] + 1, 1e-6);
  double i0n = et.f(0, EF_K0, negSOC) * sqrt(te1 * (1 - th0) * th0);  // OB_step.m:329-332
  double i0p = et.f(1, EF_K0, posSOC) * sqrt(teE * (1 - th3) * th3);
  double negEta0 = 2 * r.R * T / r.F * dasinh(yk[R_IF0] / (2 * i0n));
  double posEta3 = 2 * r.R * T / r.F * dasinh(yk[R_IF3] / (2 * i0p));
  double Uocpn0 = et.f(0, EF_U, th0), Uocpp3 = et.f(1, EF_U, th3);
  const double Rfn = et.f(0, EF_RF, negSOC), Rfp = et.f(1, EF_RF, posSOC);  // OB_step.m:339-340
  double V = posEta3 - negEta0 + yk[R_PHIE] + Uocpp3 - Uocpn0 + (Rfp * yk[R_IFDL3] - Rfn * yk[R_IFDL0]);
  return V - r.Rc * Iapp;
}

// ---------------------------------------------------------------------------
// k_plant4: OB_step simStep outputs for every cell, a lane quad per cell, lane j = corner j
// of OB_step.m:251-275.  A lane per cell runs 65,536 cells as one wave per SIMD, so every
// round trip (the per-cell scalars, then the corner gathers they select) and every dependent
// FP64 chain is exposed (60 % of its cycles in s_waitcnt, VALU 15 %).  Here lane j gathers and
// replays only its corner's 48-B state and forms its 9 output rows; the blend of
// OB_step.m:281-285 takes the four corners' rows by DPP quad broadcasts in the one-lane
// expression order, and the per-cell scalar chain (bracket, clamps, asinh, Vcell) is the
// same instruction stream for the whole quad.  1024-thread blocks: 256 cells share one
// staged plant blob per CU at 4 waves per SIMD.
// ---------------------------------------------------------------------------
constexpr int PLANT4_BLOCK = 1024;
template <bool GR, bool PL>
__global__ void __launch_bounds__(PLANT4_BLOCK) k_plant4(const KRom r, const KState s, const double *iapp,
                                                         double *vout, const int lazy_t, const double *tc_in) {
  extern __shared__ double lds[];
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (int)(gt & 3);
  const int64_t c = gt >> 2;  // a quad is one cell: every exit below is quad-uniform
#ifdef MPCEKF_STAMPS
  if (c < s.n && j == 0 && s.stamps) s.stamps[(size_t)19 * s.n + c] = (long long)__builtin_amdgcn_s_memtime();
#endif
  const int lo = GR ? r.plant_tab : 0;
  stage_lds(lds, r.plant_blob + lo, r.plant_len - lo);
  __syncthreads();
  const double *tb = lds - lo;
  const double *L = GR ? r.plant_blob : lds;
  const double *Tp = tb + r.plant_tab + r.plant_tablen;
  const double *Zp = Tp + MAXT;
  if (gt == 0 && lazy_t) *s.hslow = 0;  // k_hild_slow of the previous step has finished
  if (c >= s.n) return;
  STAMPP(0);
  const double Iapp = iapp[c];
  const double tcs = tc_in ? tc_in[c] : s.Tc[c];
  const double priorI = s.priorI[c];
  const int status = s.status[c];
  double SOCnAvg = s.SOCn[c], SOCpAvg = s.SOCp[c];
  const double SOC0n = s.SOC0n[c], SOC0p = s.SOC0p[c];
  if (j == 0) {
    if (tc_in) s.Tc[c] = tcs;  // this step's TC (runMPC.m:85-92), read by every later kernel
    if (lazy_t) {  // this step's inputs, for the deferred updates of every model (k_cell, k_flush)
      const size_t slot = (size_t)(lazy_t % LAZY_H) * s.n + c;
      s.hist_u[slot] = Iapp;
      s.hist_p[slot] = priorI;
    }
  }
  if (status & ST_ERROR) {
    if (j == 0) vout[c] = __builtin_nan("");
    return;
  }
  const double T = tcs + 273.15;  // OB_step.m:75
  const ETab et = etab<PL>(r, tb + r.plant_tab, T);
  const double negSOC = SOCnAvg, posSOC = SOCpAvg;  // obs.negSOC / posSOC: pre-update (OB_step.m:226-227)
  double cellSOC = (SOCnAvg - r.th0n) / (r.th100n - r.th0n);
  const PlantCorners pc = plant_corners(r, Tp, Zp, cellSOC, T);
  STAMPP(1);
  const int mj = corner_model(r, pc, j);  // this lane's corner
  double *bx = s.bigx + ((size_t)c * r.NM + mj) * 6;
  double xs[6];
  load_corner(bx, xs);
  const int tsj = lazy_t ? s.ts_plant[c * r.NM + mj] : 0;
  // the per-cell scalar chain runs while the corner gathers are in flight
  plant_soc_step(r, et, SOC0n, SOC0p, Iapp, SOCnAvg, SOCpAvg);
  double aZ, aT;
  plant_weights(Tp, Zp, pc, cellSOC, T, aZ, aT);
  STAMPP(2);
  const double *a = L + mj * PREC + NPLANT * NX + 2 * NPLANT;
  if (lazy_t) plant_replay<true>(xs, a, s, c, tsj, lazy_t);
  STAMPP(3);
  const double *B = L + mj * PREC;
  double yk[NPLANT];
#pragma unroll
  for (int q = 0; q < NPLANT; ++q) {
    yk[q] = quad_blend(plant_row(B + q * NX, B[NPLANT * NX + q], B[NPLANT * NX + NPLANT + q], xs, Iapp), aZ, aT);
    __builtin_amdgcn_sched_barrier(0);  // one row's LDS operands at a time: 128 VGPRs at 4 waves/SIMD
  }
  STAMPP(4);
  const double V = plant_vcell(r, et, yk, T, Iapp, negSOC, posSOC, SOC0n, SOC0p);
  STAMPP(5);
  if (j == 0) {
    s.SOCn[c] = SOCnAvg;
    s.SOCp[c] = SOCpAvg;
    vout[c] = V;
  }
  // advance this corner through step t in place (eager mode: k_bulk does all models); a
  // duplicate corner (single-set-point grids) is written by two lanes with the same bits
  if (lazy_t && tsj < lazy_t) {
    double x[6];
    plant_advance<true>(a, xs, Iapp, x);
    store_corner(bx, x);
    s.ts_plant[c * r.NM + mj] = lazy_t;
  }
  STAMPP(6);
}

// ---------------------------------------------------------------------------
// k_plant_obs: every observable of OB_step.m:226-228,289-356 for the stage route
// (mpcekf_plant_step_obs), a lane quad per cell as k_plant4.  It is launched BEFORE the
// call's k_plant4 / k_bulk and only reads the plant state (SOCn/SOCp, bigx at step t-1), so
// Vcell and the state the call leaves are k_plant4's own; this kernel recomputes Vcell with
// the shared plant helpers (the same bits) for posPhis and the record's Vcell slot.
// The obs blob (host build_rom) holds, per model, all nz rows in the permuted order as
// [C 5][res0][D][0] -- res0 zeroed on the Phise rows, OB_step.m:178-181 -- then the plant
// blob's tables.  Pass 1 forms role rows 0..R_PHISE0 (unrolled, registers) for Vcell and
// negPhise0; pass 2 walks every row once more: blend, the row's correction (OBS_* kind) and
// its one or two record slots, all from the row's uniform descriptor word.  The record is
// slot-major [nobs][n]; lane j of the quad stores the slots = j (mod 4).
// ---------------------------------------------------------------------------
// The prologue of the two obs kernels.  obs_stage: the block's obs blob in LDS (GR: tables
// only, model rows from the global blob).  obs_cell: lane j's view of cell c at temperature T,
// from the pre-update averages through the blend weights; *tsj, where asked for, is the step
// the corner's stored state is current through.
struct ObsBlob {
  const double *tb, *L, *Tp, *Zp;
};
template <bool GR>
__device__ __forceinline__ ObsBlob obs_stage(const KObs &o, double *lds) {
  const int lo = GR ? o.tab : 0;
  stage_lds(lds, o.blob + lo, o.len - lo);
  __syncthreads();
  const double *tb = lds - lo;
  const double *Tp = tb + o.tab + o.tablen;
  return {tb, GR ? o.blob : lds, Tp, Tp + MAXT};
}
struct ObsCell {
  double negSOC, posSOC, SOC0n, SOC0p, cellSOC, aZ, aT;
  ETab et;
  double xs[6];     // lane j's corner state
  const double *B;  // and its rows of the obs blob
  int mj;
};
template <bool PL>
__device__ __forceinline__ void obs_cell(const KRom &r, const KState &s, const KObs &o, const ObsBlob &ob, int64_t c,
                                         int j, double T, ObsCell &k, int *tsj = nullptr) {
  k.negSOC = s.SOCn[c], k.posSOC = s.SOCp[c];  // OB_step.m:226-227
  k.SOC0n = s.SOC0n[c], k.SOC0p = s.SOC0p[c];
  k.et = etab<PL>(r, ob.tb + o.tab, T);
  k.cellSOC = (k.negSOC - r.th0n) / (r.th100n - r.th0n);  // OB_step.m:228
  const PlantCorners pc = plant_corners(r, ob.Tp, ob.Zp, k.cellSOC, T);
  k.mj = corner_model(r, pc, j);
  // along the fused loop (tsj: k_obs_traj) the corner may be held in the plant window, where
  // k_cell's cell_plant left it at step t - 1; the stage route never meets a held slot
  const int slot = tsj && s.hotp_m ? hotp_find(s, c, k.mj) : -1;
  load_corner(slot >= 0 ? hotp_slot(s, slot, c) : s.bigx + ((size_t)c * r.NM + k.mj) * 6, k.xs,
              slot >= 0 ? (size_t)s.n : 1);
  if (tsj) *tsj = *(slot >= 0 ? s.hotp_ts + (size_t)slot * s.n + c : s.ts_plant + c * r.NM + k.mj);
  plant_weights(ob.Tp, ob.Zp, pc, k.cellSOC, T, k.aZ, k.aT);
  k.B = ob.L + (size_t)k.mj * o.stride;
}
// a blended row's correction by its OBS_* kind (OB_step.m:302-326, 348)
__device__ __forceinline__ double obs_correct(int kind, double v, const ObsCell &k, double UocpnAvg, double UocppAvg,
                                              double negPhise0, double V) {
  switch (kind) {
    case OBS_NTHSS: return fmin(fmax(v + k.SOC0n, 1e-6), 1 - 1e-6);  // OB_step.m:302-310
    case OBS_PTHSS: return fmin(fmax(v + k.SOC0p, 1e-6), 1 - 1e-6);
    case OBS_NPHISE: return v + UocpnAvg;                            // OB_step.m:315-317
    case OBS_PPHISE: return v + UocppAvg;
    case OBS_PHIE: return v - negPhise0;                             // OB_step.m:322
    case OBS_THETAE: return fmax(v + 1, 1e-6);                       // OB_step.m:325-326
    case OBS_PPHIS: return v + V;                                    // OB_step.m:348
    default: return v;
  }
}
constexpr int OBS_BLOCK = 512;  // 256 VGPRs a lane: no scratch (at 1024 / 128 the quintic lookups spilled)
template <bool GR, bool PL>
__global__ void __launch_bounds__(OBS_BLOCK) k_plant_obs(const KRom r, const KState s, const KObs o,
                                                            const double *iapp) {
  extern __shared__ double lds[];
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (int)(gt & 3);
  const int64_t c = gt >> 2;  // a quad is one cell: every exit below is quad-uniform
  const ObsBlob ob = obs_stage<GR>(o, lds);
  if (c >= s.n) return;
  const size_t n = (size_t)s.n;
  double *rec = o.rec + c;
  auto put = [&](int slot, double v) {
    if ((slot & 3) == j) rec[(size_t)slot * n] = v;
  };
  if (s.status[c] & ST_ERROR) {
    for (int k = j; k < o.nobs; k += 4) rec[(size_t)k * n] = __builtin_nan("");
    return;
  }
  const double Iapp = iapp[c];
  const double T = s.Tc[c] + 273.15;  // OB_step.m:75
  ObsCell k;
  obs_cell<PL>(r, s, o, ob, c, j, T, k);
  double yk[R_PHISE0 + 1];
#pragma unroll
  for (int q = 0; q <= R_PHISE0; ++q) {
    yk[q] = quad_blend(obs_row(k.B + q * OBS_ROW, k.xs, Iapp), k.aZ, k.aT);
    __builtin_amdgcn_sched_barrier(0);  // one row's operands at a time (k_plant4)
  }
  const double V = plant_vcell(r, k.et, yk, T, Iapp, k.negSOC, k.posSOC, k.SOC0n, k.SOC0p);
  __builtin_amdgcn_sched_barrier(0);  // Vcell's lookups done before the two of the averages start
  const double UocpnAvg = k.et.f(0, EF_U, k.negSOC), UocppAvg = k.et.f(1, EF_U, k.posSOC);  // OB_step.m:313-314
  const double negPhise0 = yk[R_PHISE0] + UocpnAvg;                                         // OB_step.m:317
  __builtin_amdgcn_sched_barrier(0);
  put(OBS_S_NEGSOC, k.negSOC);
  put(OBS_S_POSSOC, k.posSOC);
  put(OBS_S_CELLSOC, k.cellSOC);
  put(o.slot_phie0, -negPhise0);  // OB_step.m:321
  put(o.nobs - 1, V);             // OB_step.m:356
  for (int q = 0; q < r.nz; ++q) {
    const unsigned d = o.desc[q];
    const int kind = (int)(d & 15u), s1 = (int)(d >> 4 & 1023u) - 1, s2 = (int)(d >> 14 & 1023u) - 1;
    if (s1 < 0 && s2 < 0) continue;  // a Phie row at x = 0 (OB_step.m:151-155): in no field
    const double v = obs_correct(kind, quad_blend(obs_row(k.B + q * OBS_ROW, k.xs, Iapp), k.aZ, k.aT), k, UocpnAvg,
                                 UocppAvg, negPhise0, V);
    if (s1 >= 0) put(s1, v);
    if (s2 >= 0) put(s2, v);
  }
}

// ---------------------------------------------------------------------------
// k_obs_traj: selected observables of OB_step.m:226-228,289-356 along the fused loop
// (mpcekf_step_ex_obs), k_plant_obs's lane quad on k_plant_obs's blob.  Launched at the top
// of fused step t, before whichever kernel runs the plant (k_plant4, k_cell's cell_plant,
// k_ekf4's quad_plant); it only reads the state and stores nothing but its output rows.
//  - The fused loop defers the all-model time update: lane j's corner record is current
//    through step ts_plant[c][mj] of the running call, so the lane replays it through steps
//    ts + 1 .. t - 1 from the hist_u ring in registers, with the plant's own expression
//    (k_plant4) and diag(A) of the plant blob: the plant's bits, and no store to bigx.
//  - The step's inputs: Iapp = s.uk (the command the step applies) and the temperature of
//    tc_in, which no kernel has written to s.Tc yet.
//  - Only the call's selected slots: q.plan[p] is the source of output position p (a
//    permuted row, or SRC_* below), so a row no position reads is never formed, and q.need
//    (wave-uniform) skips the Vcell chain and the two average-Uocp lookups nobody asked for.
// Output position p of this step at q.out[p * n + c], stored by lane p & 3 of the quad.
// Every value: k_plant_obs's expressions, hence its bits.
// ---------------------------------------------------------------------------
template <bool GR, bool PL>
__global__ void __launch_bounds__(OBS_BLOCK) k_obs_traj(const KRom r, const KState s, const KObs o, const KObsSel q,
                                                           const int lazy_t, const double *tc_in) {
  extern __shared__ double lds[];
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (int)(gt & 3);
  const int64_t c = gt >> 2;  // a quad is one cell: every exit below is quad-uniform
  const ObsBlob ob = obs_stage<GR>(o, lds);
  if (c >= s.n) return;
  const size_t n = (size_t)s.n;
  double *out = q.out + c;
  if (s.status[c] & ST_ERROR) {
    for (int p = j; p < q.nsel; p += 4) out[(size_t)p * n] = __builtin_nan("");
    return;
  }
  const double Iapp = s.uk[c];
  const double T = (tc_in ? tc_in[c] : s.Tc[c]) + 273.15;  // OB_step.m:75
  ObsCell k;
  int tsj;
  obs_cell<PL>(r, s, o, ob, c, j, T, k, &tsj);
  if (tsj + 1 < lazy_t) {  // OB_step.m:198-200 for the skipped steps
    double a[6];
    {
      const double *ap = r.plant_blob + (size_t)k.mj * PREC + NPLANT * NX + 2 * NPLANT;  // diag(A), a[5] = 1
#pragma unroll
      for (int e = 0; e < 6; ++e) a[e] = ap[e];
    }
    plant_replay<true>(k.xs, a, s, c, tsj, lazy_t);
  }
  double V = 0.0, UocpnAvg = 0.0, UocppAvg = 0.0, negPhise0 = 0.0;
  if (q.need & OBS_NEED_V) {  // the Vcell chain of k_plant4 / k_plant_obs
    double yk[R_PHIE + 1];
#pragma unroll
    for (int i = 0; i <= R_PHIE; ++i) {
      yk[i] = quad_blend(obs_row(k.B + i * OBS_ROW, k.xs, Iapp), k.aZ, k.aT);
      __builtin_amdgcn_sched_barrier(0);  // one row's operands at a time (k_plant4)
    }
    V = plant_vcell(r, k.et, yk, T, Iapp, k.negSOC, k.posSOC, k.SOC0n, k.SOC0p);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (q.need & OBS_NEED_UN) {  // OB_step.m:313,317
    UocpnAvg = k.et.f(0, EF_U, k.negSOC);
    negPhise0 = quad_blend(obs_row(k.B + R_PHISE0 * OBS_ROW, k.xs, Iapp), k.aZ, k.aT) + UocpnAvg;
    __builtin_amdgcn_sched_barrier(0);
  }
  if (q.need & OBS_NEED_UP) {  // OB_step.m:314
    UocppAvg = k.et.f(1, EF_U, k.posSOC);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int p = 0; p < q.nsel; ++p) {
    const int src = q.plan[p];  // wave-uniform
    double v;
    if (src >= 0) {
      v = obs_correct((int)(o.desc[src] & 15u), quad_blend(obs_row(k.B + src * OBS_ROW, k.xs, Iapp), k.aZ, k.aT), k,
                      UocpnAvg, UocppAvg, negPhise0, V);
    } else {
      v = src == OBS_SRC_NEGSOC ? k.negSOC : src == OBS_SRC_POSSOC ? k.posSOC : src == OBS_SRC_CELLSOC ? k.cellSOC
          : src == OBS_SRC_PHIE0 ? -negPhise0 : V;  // OB_step.m:226-228, 321, 356
    }
    if ((p & 3) == j) out[(size_t)p * n] = v;
  }
}

// ---------------------------------------------------------------------------
// k_bulk: all-model plant advance and EKF time update (HBM streaming)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bulk(const KRom r, const KCfg cf, const KState s, const double *iapp,
                                              int do_plant, int do_ekf) {
  extern __shared__ double lds[];
  const int NM = r.NM;
  const int ne = NM * REC, np = NM * 6;
  stage_lds(lds, r.bulk_tab, ne + np);
  __syncthreads();
  const double *cC = lds, *cP = lds + ne;
  const double W = cf.SigmaW;
  for (int64_t c = blockIdx.x; c < s.n; c += gridDim.x) {
    if (do_ekf) {
      double pri = s.priorI[c];
      double2 *base = reinterpret_cast<double2 *>(s.ekf + (size_t)c * ne);
      for (int j = threadIdx.x; j < ne / 2; j += blockDim.x) {
        int e0 = (2 * j) % REC;
        double2 v = base[j];
        double add0 = e0 < NX ? pri : W;
        double add1 = e0 + 1 < NX ? pri : W;
        v.x = __builtin_fma(cC[2 * j], v.x, add0);
        v.y = __builtin_fma(cC[2 * j + 1], v.y, add1);
        base[j] = v;
      }
    }
    if (do_plant) {
      double u = iapp[c];
      double2 *base = reinterpret_cast<double2 *>(s.bigx + (size_t)c * np);
      for (int j = threadIdx.x; j < np / 2; j += blockDim.x) {
        double2 v = base[j];
        v.x = __builtin_fma(cP[2 * j], v.x, u);
        v.y = __builtin_fma(cP[2 * j + 1], v.y, u);
        base[j] = v;
      }
    }
  }
}

// k_flush: brings every local model (EKF record and plant state) of every cell
// from its timestamp to step t with the logged inputs, then stamps it new_ts.
// Block per cell, the cell's input rings and timestamps staged in LDS.
// Lane per model: a wave takes one cell at a time (grid-stride) with its lanes on
// models m0 + lane; the model's coefficients (diag(A) for xhat, a_p a_q for Sigma, bigA
// for the plant) stay in registers across cells, the record (26 doubles) is loaded once,
// replayed step by step and stored once.  The step inputs come from the lane holding
// that ring slot (readlane; k is wave-uniform), so a step is 26 FMAs and no memory.
__device__ __forceinline__ double rl64(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__global__ void __launch_bounds__(256) k_flush(const KRom r, const KCfg cf, const KState s, const int t,
                                               const int new_ts, const int64_t c_lo, const int64_t c_hi) {
  const int NM = r.NM;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const double W = cf.SigmaW;
  const double *cC = r.bulk_tab, *cP = r.bulk_tab + (size_t)NM * REC;
  for (int m0 = 0; m0 < NM; m0 += 64) {
    const int m = m0 + lane;
    const bool act = m < NM;
    const int mm = act ? m : NM - 1;
    double ce[REC], cp[6];
#pragma unroll
    for (int e = 0; e < REC; ++e) ce[e] = cC[(size_t)mm * REC + e];
#pragma unroll
    for (int e = 0; e < 6; ++e) cp[e] = cP[(size_t)mm * 6 + e];
    // software pipelined over the wave's cells: the next cell's rings, timestamps and
    // records are loaded while this cell replays, so every wave keeps a cell's 13.6 KB
    // in flight
    struct FCell {
      double hpl, hul, xe[REC], xp[6];
      int tse, tsp;
      int slot;   // the corner-window slot that holds this lane's model, -1: its record is in s.ekf
      int pslot;  // the plant-window slot that holds it, -1: its plant state is in s.bigx
    };
    // the cell's eight window tags in one load (lanes 0..3 the corner window's, 4..7 the plant
    // window's; -1 where there is no window), taken one cell ahead of the records: the slot, and
    // with it the address of every record load, then depends on no load of the same stage
    const int *tags = lane < 4 ? s.hot_m : s.hotp_m;
    auto ftag = [&](int64_t c) -> int { return lane < 8 && tags ? tags[(size_t)(lane & 3) * s.n + c] : -1; };
    auto fload = [&](int64_t c, FCell &F, const int tag) {
      F.hpl = s.hist_p[(size_t)(lane & (LAZY_H - 1)) * s.n + c];
      F.hul = s.hist_u[(size_t)(lane & (LAZY_H - 1)) * s.n + c];
      // the tags handed round by readlane: the lane whose model a slot holds takes the record (the
      // plant state) and its timestamp from that slot
      F.slot = -1;
      F.pslot = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (act && __builtin_amdgcn_readlane(tag, j) == m) F.slot = j;
        if (act && __builtin_amdgcn_readlane(tag, 4 + j) == m) F.pslot = j;
      }
      const int *tp = F.slot >= 0 ? s.hot_ts + (size_t)F.slot * s.n + c : s.ts_ekf + c * NM + mm;
      const int *tq = F.pslot >= 0 ? s.hotp_ts + (size_t)F.pslot * s.n + c : s.ts_plant + c * NM + mm;
      // MB never time-updates the per-model EKF records (iterEKF.m:90-102)
      F.tse = (act && !(cf.flags & KF_MB)) ? *tp : t;
      F.tsp = act ? *tq : t;
      // one code path for record and slot: a per-lane pointer that steps by the pair stride (1 on
      // a record, n in a window), an add per pair and no per-lane multiply
      const double2 *re = reinterpret_cast<const double2 *>(F.slot >= 0 ? hot_slot(s, F.slot, c)
                                                                        : s.ekf + ((size_t)c * NM + mm) * REC);
      const double2 *rp = reinterpret_cast<const double2 *>(F.pslot >= 0 ? hotp_slot(s, F.pslot, c)
                                                                         : s.bigx + ((size_t)c * NM + mm) * 6);
      const size_t rst = F.slot >= 0 ? (size_t)s.n : 1, pst = F.pslot >= 0 ? (size_t)s.n : 1;
#pragma unroll
      for (int e = 0; e < REC / 2; ++e, re += rst) {
        const double2 v = *re;
        F.xe[2 * e] = v.x;
        F.xe[2 * e + 1] = v.y;
      }
#pragma unroll
      for (int e = 0; e < 3; ++e, rp += pst) {
        const double2 v = *rp;
        F.xp[2 * e] = v.x;
        F.xp[2 * e + 1] = v.y;
      }
    };
    FCell cur;
    int tagn = -1;  // the tags of the cell the next fload takes
    if (c_lo + w0 < c_hi) {
      fload(c_lo + w0, cur, ftag(c_lo + w0));
      if (c_lo + w0 + nw < c_hi) tagn = ftag(c_lo + w0 + nw);
    }
    for (int64_t c = c_lo + w0; c < c_hi; c += nw) {
      FCell nx;
      if (c + nw < c_hi) {
        const int tag = tagn;
        if (c + 2 * nw < c_hi) tagn = ftag(c + 2 * nw);
        fload(c + nw, nx, tag);
      }
      const double hpl = cur.hpl, hul = cur.hul;
      const int tse = cur.tse, tsp = cur.tsp;
      double2 *re = reinterpret_cast<double2 *>(s.ekf + ((size_t)c * NM + mm) * REC);
      double2 *rp = reinterpret_cast<double2 *>(s.bigx + ((size_t)c * NM + mm) * 6);
      double *xe = cur.xe, *xp = cur.xp;
      int kmin = min(tse, tsp);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) kmin = min(kmin, __shfl_xor(kmin, o));
      for (int k = kmin + 1; k <= t; ++k) {  // k is wave-uniform
        const int sl = k & (LAZY_H - 1);
        const double p = rl64(hpl, sl), u = rl64(hul, sl);
        if (k > tse) {
#pragma unroll
          for (int e = 0; e < NX; ++e) xe[e] = __builtin_fma(ce[e], xe[e], p);
#pragma unroll
          for (int e = NX; e < REC; ++e) xe[e] = __builtin_fma(ce[e], xe[e], W);
        }
        if (k > tsp) {
#pragma unroll
          for (int e = 0; e < 6; ++e) xp[e] = __builtin_fma(cp[e], xp[e], u);
        }
      }
      // a record held in the corner window goes back to s.ekf even when it is current (the
      // copy there is stale), and its slot is left empty
      if (tse < t || cur.slot >= 0) {
#pragma unroll
        for (int e = 0; e < REC / 2; ++e) re[e] = make_double2(xe[2 * e], xe[2 * e + 1]);
      }
      if (cur.slot >= 0) s.hot_m[(size_t)cur.slot * s.n + c] = -1;
      // the same for a plant state held in the plant window
      if (cur.pslot >= 0) s.hotp_m[(size_t)cur.pslot * s.n + c] = -1;
      if (tsp < t || cur.pslot >= 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e) rp[e] = make_double2(xp[2 * e], xp[2 * e + 1]);
      }
      if (act) {
        s.ts_ekf[c * NM + m] = new_ts;
        s.ts_plant[c * NM + m] = new_ts;
      }
      cur = nx;
    }
  }
}

// ---------------------------------------------------------------------------
// Deferred time update (fused mpcekf_step): iterEKF.m:73-84 for the steps model m
// skipped, replayed in the per-step order of the eager update (k_bulk / the oracle),
// so the record is bit-identical to one advanced every step.
// ---------------------------------------------------------------------------
// The skipped time updates of one model, steps ts+1..t (pt = the step-t input).
__device__ __forceinline__ void replay_x(double x[NX], const double *a, int ts, int t, double pt, const KState &s,
                                        int64_t c) {
  if (ts + 1 < t) {  // steps before t: their inputs from the ring
    for (int k0 = ts + 1; k0 < t; k0 += RCH) {
      double p[RCH];
      ring_chunk(s.hist_p, s, c, k0, t - 1, p);
#pragma unroll
      for (int i = 0; i < RCH; ++i)
        if (k0 + i < t)
#pragma unroll
          for (int e = 0; e < NX; ++e) x[e] = __builtin_fma(a[e], x[e], p[i]);
    }
  }
  if (ts < t)
#pragma unroll
    for (int e = 0; e < NX; ++e) x[e] = __builtin_fma(a[e], x[e], pt);
}
// a: the model's diag(A) [NX] followed by its a_p a_q coefficients [NPK] (cell blob)
__device__ __forceinline__ void replay_S(double S[NPK], const double *a, int ts, int t, double W) {
  for (int k = ts + 1; k <= t; ++k) {
#pragma unroll
    for (int i = 0, pp = 0; pp < NX; ++pp)
#pragma unroll
      for (int q = pp; q < NX; ++q, ++i) S[i] = __builtin_fma(a[NX + i], S[i], W);
  }
}

template <int NZ>
__device__ __forceinline__ void ekf_catch_up4(const KState &s, const CellCtx &cc, int NM, const int m[4], int64_t c,
                                              int t, double W, double pt, const bool held[4]) {
  // all timestamps, then all lagging records, in flight together (latency, not bytes,
  // is the cost here); a model named by several corners is advanced once.  held[j]: the
  // model is current in the corner window (its s.ekf record and timestamp are stale)
  int ts[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ts[j] = held[j] ? t : s.ts_ekf[c * NM + m[j]];
  bool need[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    need[j] = ts[j] < t;
#pragma unroll
    for (int i = 0; i < j; ++i) need[j] = need[j] && m[i] != m[j];
  }
  if (!(need[0] || need[1] || need[2] || need[3])) return;
  // pt: step t's input (the ring's slot t, which k_cell stores only after its last load)
  double x[4][NX], S[4][NPK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (need[j]) load_rec(cc.erec + (size_t)m[j] * REC, x[j], S[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!need[j]) continue;
    const double *a = cc.L + m[j] * cc.stride + NZ * NX + NZ;  // diag(A) of the model (cell blob)
    for (int k0 = ts[j] + 1; k0 <= t; k0 += RCH) {
      double p[RCH];
      if (k0 < t) ring_chunk(s.hist_p, s, c, k0, t - 1, p);
#pragma unroll
      for (int i = 0; i < RCH; ++i) {
        const int k = k0 + i;
        if (k > t) break;
        const double pk_ = k == t ? pt : p[i];
#pragma unroll
        for (int e = 0; e < NX; ++e) x[j][e] = __builtin_fma(a[e], x[j][e], pk_);
#pragma unroll
        for (int q = 0; q < NPK; ++q) S[j][q] = __builtin_fma(a[NX + q], S[j][q], W);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (need[j]) {
      store_rec(cc.erec + (size_t)m[j] * REC, x[j], S[j]);
      s.ts_ekf[c * NM + m[j]] = t;
    }
}

// ---------------------------------------------------------------------------
// Model blend ('MB', initKF.m:44-49): one blended model per cell, its (n+1) state and
// full 6x6 covariance in s.mb [n][MBREC] = xhat[0..4], -, Sigma 6x6 row-major; the
// integrator xhat(end) lives in s.x0.  The sequence is oracle/mpcekf_oracle.c
// ekf_step_mb / meas_cov_mb / get_chat_v_mb, operation for operation.
// ---------------------------------------------------------------------------
constexpr int NA6 = NX + 1;
constexpr int NPK6 = NA6 * (NA6 + 1) / 2;
__device__ __forceinline__ int pk6(int r, int c) {
  return r <= c ? r * NA6 - (r * (r - 1)) / 2 + (c - r) : c * NA6 - (c * (c - 1)) / 2 + (r - c);
}

// getChatV 'MB' (iterEKF.m:448-459, 475-479, 489-491, 512-517): the gamma-weighted sums
// of the four corners' rows, then the terms; the integrator entry last.
template <int NZ>
__device__ __forceinline__ void chat_mb(const KRom &r, const CellCtx &cc, const XI &xi, double xSOC, double zTE1,
                                        double zTH0, double zTEE, double zTH3, double ChV[NA6]) {
  const ChatK K = chat_k(r, cc, xSOC, zTE1, zTH0, zTEE, zTH3);
  constexpr int rows[7] = {R_IFDL3, R_IFDL0, R_IF3, R_IF0, R_PHIE, R_TH3, R_TH0};
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    double sum[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) a = a + xi.g[j] * cc.L[xi.m[j] * cc.stride + rows[t] * NX + k];
      sum[t] = a;
    }
    double v = K.Rfp * sum[0] - K.Rfn * sum[1];
    v = v + K.Rctp * sum[2] - K.Rctn * sum[3];
    v = v + sum[4];
    v = v + K.dUp3 * sum[5] - K.dUn0 * sum[6];
    ChV[k] = v;
  }
  ChV[NX] = chat0(r, K);
}

// row' * Sigma * row on the full 6x6 (orc qform_full): t_c = sum_k fma(S_kc, row_k),
// acc = sum_c fma(t_c, row_c)
__device__ __forceinline__ double qform6(const double S[NA6 * NA6], const double row[NA6]) {
  double acc = 0.0;
#pragma unroll
  for (int cI = 0; cI < NA6; ++cI) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < NA6; ++k) t = __builtin_fma(S[k * NA6 + cI], row[k], t);
    acc = __builtin_fma(t, row[cI], acc);
  }
  return acc;
}

__device__ __forceinline__ bool is_pd6(const double a[NPK6]) {  // orc is_pd_n(6)
  double l[NA6][NA6], d[NA6];
  bool pd = true;
#pragma unroll
  for (int j = 0; j < NA6; ++j) {
    double sj = a[pk6(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) sj = __builtin_fma(-(l[j][k] * l[j][k]), d[k], sj);
    pd = pd && (sj > 0);
    d[j] = sj;
    const double inv = 1.0 / sj;
#pragma unroll
    for (int i = j + 1; i < NA6; ++i) {
      double t = a[pk6(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) t = __builtin_fma(-(l[i][k] * l[j][k]), d[k], t);
      l[i][j] = t * inv;
    }
  }
  return pd;
}

__device__ __noinline__ void jacobi6(double a[NPK6], double V[NA6 * NA6]) {  // orc_jacobi(6), packed
#pragma unroll
  for (int i = 0; i < NA6 * NA6; ++i) V[i] = (i % (NA6 + 1)) == 0 ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int p = 0; p < NA6; ++p) {
      dg = dg + a[pk6(p, p)] * a[pk6(p, p)];
#pragma unroll
      for (int q = p + 1; q < NA6; ++q) off = off + a[pk6(p, q)] * a[pk6(p, q)];
    }
    if (!(off > 1e-36 * dg)) break;
#pragma unroll
    for (int p = 0; p < NA6 - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < NA6; ++q) {
        double apq = a[pk6(p, q)];
        if (apq != 0.0) {
          double theta = (a[pk6(q, q)] - a[pk6(p, p)]) / (2.0 * apq);
          double t;
          if (fabs(theta) > 1e150) {
            t = 0.5 / theta;
          } else {
            t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0) t = -t;
          }
          double c = 1.0 / sqrt(t * t + 1.0), sn = t * c, tau = sn / (1.0 + c);
          a[pk6(p, p)] = a[pk6(p, p)] - t * apq;
          a[pk6(q, q)] = a[pk6(q, q)] + t * apq;
          a[pk6(p, q)] = 0.0;
#pragma unroll
          for (int rr = 0; rr < NA6; ++rr) {
            if (rr == p || rr == q) continue;
            double g = a[pk6(rr, p)], h = a[pk6(rr, q)];
            a[pk6(rr, p)] = g - sn * (h + g * tau);
            a[pk6(rr, q)] = h + sn * (g - h * tau);
          }
#pragma unroll
          for (int rr = 0; rr < NA6; ++rr) {
            double g = V[rr * NA6 + p], h = V[rr * NA6 + q];
            V[rr * NA6 + p] = g - sn * (h + g * tau);
            V[rr * NA6 + q] = h + sn * (g - h * tau);
          }
        }
      }
    }
  }
}

// iterEKF.m:164-173 on the full MB covariance (orc meas_cov_mb)
__device__ __forceinline__ void meas_cov_mb(double S[NA6 * NA6], const double L[NA6], double St, bool bump) {
  double P[NA6 * NA6], a[NPK6];
#pragma unroll
  for (int rr = 0; rr < NA6; ++rr)
#pragma unroll
    for (int cI = 0; cI < NA6; ++cI) P[rr * NA6 + cI] = __builtin_fma(-(L[rr] * St), L[cI], S[rr * NA6 + cI]);
#pragma unroll
  for (int rr = 0; rr < NA6; ++rr)
#pragma unroll
    for (int cI = rr; cI < NA6; ++cI) a[pk6(rr, cI)] = (P[rr * NA6 + cI] + P[cI * NA6 + rr]) * 0.5;
  if (is_pd6(a)) {
#pragma unroll
    for (int rr = 0; rr < NA6; ++rr)
#pragma unroll
      for (int cI = rr; cI < NA6; ++cI) {
        double v = (((P[rr * NA6 + cI] + P[cI * NA6 + rr]) + a[pk6(rr, cI)]) + a[pk6(rr, cI)]) / 4.0;
        if (bump) v = v * 2.0;
        S[rr * NA6 + cI] = v;
        S[cI * NA6 + rr] = v;
      }
    return;
  }
  double V[NA6 * NA6], w[NA6];
  jacobi6(a, V);
#pragma unroll
  for (int k = 0; k < NA6; ++k) w[k] = fabs(a[pk6(k, k)]);
#pragma unroll
  for (int rr = 0; rr < NA6; ++rr)
#pragma unroll
    for (int cI = rr; cI < NA6; ++cI) {
      double hrc = 0.0, hcr = 0.0;
#pragma unroll
      for (int k = 0; k < NA6; ++k) {
        hrc = hrc + (V[rr * NA6 + k] * w[k]) * V[cI * NA6 + k];
        hcr = hcr + (V[cI * NA6 + k] * w[k]) * V[rr * NA6 + k];
      }
      double v = (((P[rr * NA6 + cI] + P[cI * NA6 + rr]) + hrc) + hcr) / 4.0;
      if (bump) v = v * 2.0;
      S[rr * NA6 + cI] = v;
      S[cI * NA6 + rr] = v;
    }
}

// ---------------------------------------------------------------------------
// k_cell: iterEKF measurement update + EKFmatsHandler + iterMPC (lane per cell)
// ---------------------------------------------------------------------------
// row' * Sigma * row in symmetric form: T = Sigma with doubled off-diagonals,
// u_k = T_kk r_k + sum_{l>k} T_kl r_l, q = sum_k r_k u_k, explicit fma at every step
// (orc qform: 20 operations instead of the 60 of Sigma*row then row'*(.)).
__device__ __forceinline__ double qform(const double T[NPK], const double rw[NX]) {
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    double u = T[pk(k, k)] * rw[k];
#pragma unroll
    for (int l = k + 1; l < NX; ++l) u = __builtin_fma(T[pk(k, l)], rw[l], u);
    q = k == 0 ? rw[0] * u : __builtin_fma(rw[k], u, q);
  }
  return q;
}

// OB_step's simStep (OB_step.m:188-357) for one cell at the start of k_cell's fused step:
// the shared plant helpers, read from the cell blob (the plant's 9 role rows are the blob's
// first C rows, D at nzp*5, diag(A) after them -- the integrator's a = 1 exactly, checked
// by build_rom -- and the res0 column after the Sigma coefficients).  Returns Vcell; the
// plant state, averages and timestamps are stored as k_plant4 stores them; the ring inputs
// of this step (Iapp and ring_p) are left for the caller to store after its last load.
template <int NZ, bool PL>
__device__ __forceinline__ double cell_plant(const KRom &r, const KState &s, const double *L, const double *tb,
                                             const double *Tp, const double *Zp, int64_t c, int lazy_t, double Iapp,
                                             double tcs, int st, double &ring_p) {
  constexpr int OA = NZ * NX + NZ, OR0 = NZ * NX + NZ + NX + NPK, OD = NZ * NX;
  const int stride = r.cell_stride;
  if (lazy_t) ring_p = s.priorI[c];  // this step's input, for the deferred updates of every model
  if (st & ST_ERROR) return __builtin_nan("");
  const double T = tcs + 273.15;  // OB_step.m:75
  const ETab et = etab<PL>(r, tb + r.cell_tab, T);
  double SOCnAvg = s.SOCn[c], SOCpAvg = s.SOCp[c];
  const double SOC0n = s.SOC0n[c], SOC0p = s.SOC0p[c];
  const double negSOC = SOCnAvg, posSOC = SOCpAvg;  // obs.negSOC / posSOC: pre-update (OB_step.m:226-227)
  double cellSOC = (SOCnAvg - r.th0n) / (r.th100n - r.th0n);
  const PlantCorners pc = plant_corners(r, Tp, Zp, cellSOC, T);
  int mm[4];
  corner_models(r, pc, mm);
  double *bx = s.bigx + (size_t)c * r.NM * 6;
  // The plant window (KState::hotp_*), as k_cell's corner window for the EKF
  // records.  hot: this step's four states go to slots 0..3 (a cell with a repeated corner keeps
  // the record path).  hit: slot j already holds corner j's model for all four, so they are read
  // from there as well.  Any other lane first writes every held slot back to bigx / ts_plant and
  // reads its states there (a model that moves between slots at a crossing goes through its
  // record).  One code path below: a per-lane base pointer and pair stride.
  const size_t hn = (size_t)s.n;
  bool hot = false, hit = false;
  if (s.hotp_m != nullptr && lazy_t != 0) {
    int hm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) hm[j] = s.hotp_m[j * hn + c];
    hot = pc.iZu != pc.iZl && pc.iTu != pc.iTl;  // four distinct models
    hit = hot && hm[0] == mm[0] && hm[1] == mm[1] && hm[2] == mm[2] && hm[3] == mm[3];
    if (!hit) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        const int mh = s.hotp_m[j * hn + c];
        if (mh < 0) continue;
        double xh[6];
        load_corner(hotp_slot(s, j, c), xh, hn);
        store_corner(bx + (size_t)mh * 6, xh);
        s.ts_plant[c * r.NM + mh] = s.hotp_ts[j * hn + c];
        if (!hot) s.hotp_m[j * hn + c] = -1;
      }
    }
  }
  const size_t rst = hit ? hn : 1;  // pair stride of the four states' loads
  const size_t wst = hot ? hn : 1;  // and of their stores
  // the 4 corner states as of step t-1: all loads before any store (duplicate corners)
  double xs[4][6];
  int tsj[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    load_corner(hit ? hotp_slot(s, j, c) : bx + (size_t)mm[j] * 6, xs[j], rst);
    if (lazy_t) tsj[j] = *(hit ? s.hotp_ts + j * hn + c : s.ts_plant + c * r.NM + mm[j]);
  }
  // the per-cell scalar chain while the corner gathers are in flight
  plant_soc_step(r, et, SOC0n, SOC0p, Iapp, SOCnAvg, SOCpAvg);
  if (lazy_t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) plant_replay<false>(xs[j], L + mm[j] * stride + OA, s, c, tsj[j], lazy_t);
  }
  double y[4][NPLANT];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double *B = L + mm[j] * stride;
#pragma unroll
    for (int q = 0; q < NPLANT; ++q) {
      y[j][q] = plant_row(B + q * NX, B[OR0 + q], B[OD + q], xs[j], Iapp);
      launder(y[j][q]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  double aZ, aT;
  plant_weights(Tp, Zp, pc, cellSOC, T, aZ, aT);
  double yk[NPLANT];
#pragma unroll
  for (int q = 0; q < NPLANT; ++q) yk[q] = blend4(y[0][q], y[1][q], y[2][q], y[3][q], aZ, aT);
  const double V = plant_vcell(r, et, yk, T, Iapp, negSOC, posSOC, SOC0n, SOC0p);
  s.SOCn[c] = SOCnAvg;
  s.SOCp[c] = SOCpAvg;
  if (lazy_t) {  // advance the corners through step t in place
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (tsj[j] >= lazy_t) {
        // nothing to store: a slot that did not hold this corner stays empty (its state is in
        // bigx, where the lane read it), one that did keeps what it holds
        if (hot && !hit) s.hotp_m[j * hn + c] = -1;
        continue;
      }
      double x[6];
      plant_advance<false>(L + mm[j] * stride + OA, xs[j], Iapp, x);
      // to window slot j with tag mm[j] and timestamp lazy_t (a hit rewrites no tag and touches
      // no ts_plant), or to the record
      store_corner(hot ? hotp_slot(s, j, c) : bx + (size_t)mm[j] * 6, x, wst);
      *(hot ? s.hotp_ts + j * hn + c : s.ts_plant + c * r.NM + mm[j]) = lazy_t;
      if (hot && !hit) s.hotp_m[j * hn + c] = mm[j];
    }
  }
  return V;
}

template <int NZ, int PARTS, bool MB = false, bool GR = false, bool PL = false>
__global__ void __launch_bounds__(256) k_cell(const KRom r, const KCfg cf, const KState s, const KIO io) {
  extern __shared__ double lds[];
  const int lo = GR ? r.cell_tab : 0;  // GR: model rows from the global blob (k_plant4)
  stage_lds(lds, r.cell_blob + lo, r.cell_len - lo);
  __syncthreads();
  const double *tb = lds - lo;
  const double *Tp = tb + r.cell_tab + r.cell_tablen;
  const double *Zp = Tp + MAXT;
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // the plant's ring inputs for this step (stored after the cell's last load, below, so
  // that no load of the step waits for their stores)
  double ring_u = 0.0, ring_p = 0.0;
  bool ring_late = false;
  // the per-cell work as a lambda: its early exits return here, to the late ring stores
  auto body = [&]() {
  if (c >= s.n) return;
  const int nz = r.nz;
  const double NaN = __builtin_nan("");
  CellCtx cc;
  cc.L = GR ? r.cell_blob : lds;
  cc.Tp = Tp;
  cc.Zp = Zp;
  cc.erec = s.ekf + (size_t)c * r.NM * REC;
  cc.stride = r.cell_stride;
  const bool fplant = (PARTS & P_EKF) && !MB && io.plant;  // OB_step's simStep runs here (KRom::cell_plant)
  const double Tc = fplant && io.tc_in ? io.tc_in[c] : s.Tc[c];
  if (fplant && io.tc_in) s.Tc[c] = Tc;  // this step's TC (runMPC.m:85-92), read by every later kernel
  cc.T = Tc > 100 ? Tc : Tc + 273.15;  // iterEKF.m:62-66
  cc.et = etab<PL>(r, tb + r.cell_tab, cc.T);
  int st = s.status[c];
  const bool fused = io.mode & MODE_FUSED;
  if (io.mode & (MODE_MPC | MODE_FUSED)) s.hflag[c] = 0;  // set again only if hildreth.m must run
  STAMP(0);

  auto fail_outputs = [&]() {
    if (io.u) io.u[c] = NaN;
    if (io.v) io.v[c] = NaN;
    if (io.soc) io.soc[c] = NaN;
    if (io.phise) io.phise[c] = NaN;
    if (io.nexec) io.nexec[c] = 0;
    if (io.zk)
      for (int q = 0; q < nz + 2; ++q) io.zk[c * (nz + 2) + q] = NaN;
    if (io.zbk)
      for (int q = 0; q < nz + 2; ++q) io.zbk[c * (nz + 2) + q] = NaN;
    if (io.bnd) io.bnd[BD_M * s.n + c] = -1.0;  // no boundzk record: k_bounds leaves zbk NaN
    if (io.uk_out) io.uk_out[c] = NaN;
    if (io.x_out)
      for (int q = 0; q < 6; ++q) io.x_out[c * 6 + q] = NaN;
    if (io.junc_out) io.junc_out[c] = NaN;
    if (io.jfin_out) io.jfin_out[c] = NaN;
    if (io.normdu_out) io.normdu_out[c] = NaN;
    if (io.nviol_out) io.nviol_out[c] = 0;
    if (io.lin_out)
      for (int q = 0; q < 35; ++q) io.lin_out[c * 35 + q] = NaN;
    if (io.xm_out)
      for (int q = 0; q < 4; ++q) { io.xm_out[c * 4 + q] = -1; io.xg_out[c * 4 + q] = NaN; }
  };

  double Z[NZ];
  double xmax[NX];         // fused step: EKFmatsHandler's corner xhat, from the EKF's registers
  bool have_xmax = false;
  KR kr2{};               // the second getVariables' k0 / Rf (EKFmatsHandler reuses them)
  bool have_kr2 = false;
  double vhat = 0.0, Zsoc = 0.0;
  XI xi;
  double ik = 0.0, vk = 0.0;
  double vplant = 0.0;
  bool planted = false;
  // runMPC.m:85: [voltage, ...] = OB_step(uk, TC, cellState, ROM), first.  Only the first
  // call does anything; the later ones are kept because without them the compiler orders
  // the plant's replay fmas differently (same instructions, another schedule).
  auto run_plant = [&]() {
    if constexpr ((PARTS & P_EKF) && !MB) {
      if (fplant && !planted) {
        if (c == 0 && io.lazy_t) *s.hslow = 0;  // k_hild_slow of the previous step has finished
        ring_u = s.uk[c];
        vplant = cell_plant<NZ, PL>(r, s, cc.L, tb, Tp, Zp, c, io.lazy_t, ring_u, Tc, st, ring_p);
        ring_late = io.lazy_t != 0;
        s.vk[c] = vplant;
        planted = true;
      }
    }
  };
  run_plant();
  if ((PARTS & P_EKF) && (io.mode & (MODE_EKF | MODE_FUSED))) {
    if (st & ST_ERROR) {
      run_plant();
      fail_outputs();
      return;
    }
    ik = fused ? s.uk[c] : io.ik_in[c];
    vk = fused ? s.vk[c] : io.vk_in[c];  // the plant's Vcell replaces it below
    int warn = s.warn[c];
    if (warn > cf.max_warn) {  // iterEKF.m:55-59
      run_plant();
      st |= ST_LOCKOUT | ST_ERROR;
      s.status[c] = st;
      if (fused) s.uk[c] = NaN;
      fail_outputs();
      return;
    }
    if constexpr (MB) {
    run_plant();
    // iterEKF.m:90-102 ('MB' time update), 106-108, 125-128 (gain), 160-176 (update),
    // 181-183, 199-203 (boundzk); the per-model records are never touched
    const double rs = r.Ts / (3600 * r.Q);
    const double SOC0 = s.SOC0[c];
    const double pri = s.priorI[c];
    double xm[NX], Sf[NA6 * NA6];
    {
      const double2 *p = reinterpret_cast<const double2 *>(s.mb + (size_t)c * MBREC);
      double v[MBREC];
#pragma unroll
      for (int i = 0; i < MBREC / 2; ++i) { const double2 q = p[i]; v[2 * i] = q.x; v[2 * i + 1] = q.y; }
#pragma unroll
      for (int k = 0; k < NX; ++k) xm[k] = v[k];
#pragma unroll
      for (int i = 0; i < NA6 * NA6; ++i) Sf[i] = v[6 + i];
    }
    double x0 = s.x0[c];  // xhat(end)
    get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC0 - x0 * rs, xi);  // iterEKF.m:92-93
    double amb[NA6];
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) a = a + cc.L[xi.m[j] * cc.stride + NZ * NX + NZ + k] * xi.g[j];
      amb[k] = a;
    }
    amb[NX] = 1.0;
#pragma unroll
    for (int k = 0; k < NX; ++k) xm[k] = amb[k] * xm[k] + pri;
    x0 = x0 + pri;
#pragma unroll
    for (int pp = 0; pp < NA6; ++pp)
#pragma unroll
      for (int q = 0; q < NA6; ++q) Sf[pp * NA6 + q] = (amb[pp] * Sf[pp * NA6 + q]) * amb[q] + cf.SigmaW;
    get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC0 - x0 * rs, xi);
    double xr[4][NX];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NX; ++k) xr[j][k] = xm[k];
    vhat = get_vars<NZ>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xr);
    if (st & ST_ERROR) {
      s.status[c] = st;
      s.warn[c] = warn;
      if (fused) s.uk[c] = NaN;
      fail_outputs();
      return;
    }
    double ChV[NA6], Lk[NA6];
    chat_mb<NZ>(r, cc, xi, SOC0 - x0 * rs, Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3], ChV);
    const double St = qform6(Sf, ChV) + cf.SigmaV;
#pragma unroll
    for (int pp = 0; pp < NA6; ++pp) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NA6; ++k) acc = __builtin_fma(Sf[pp * NA6 + k], ChV[k], acc);
      Lk[pp] = acc / St;
    }
    const double res = vk - vhat;
#pragma unroll
    for (int k = 0; k < NX; ++k) xm[k] = __builtin_fma(Lk[k], res, xm[k]);
    x0 = __builtin_fma(Lk[NX], res, x0);
    meas_cov_mb(Sf, Lk, St, res * res > 9 * St);
    get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC0 - x0 * rs, xi);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NX; ++k) xr[j][k] = xm[k];
    vhat = get_vars<NZ>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xr);
    s.warn[c] = warn;
    {
      double2 *p = reinterpret_cast<double2 *>(s.mb + (size_t)c * MBREC);
      double v[MBREC];
#pragma unroll
      for (int k = 0; k < NX; ++k) v[k] = xm[k];
      v[NX] = 0.0;
#pragma unroll
      for (int i = 0; i < NA6 * NA6; ++i) v[6 + i] = Sf[i];
#pragma unroll
      for (int i = 0; i < MBREC / 2; ++i) p[i] = make_double2(v[2 * i], v[2 * i + 1]);
    }
    s.x0[c] = x0;
    if (st & ST_ERROR) {
      s.status[c] = st;
      if (fused) s.uk[c] = NaN;
      fail_outputs();
      return;
    }
    s.priorI[c] = ik;  // iterEKF.m:210
    if (io.zbk) {  // getChatZ 'MB' (iterEKF.m:537-538, 554-558, 575-576, 596-600) + iterEKF.m:199-203
      const double xSOC = SOC0 - x0 * rs;
      double ChVz[NA6];
      chat_mb<NZ>(r, cc, xi, xSOC, Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3], ChVz);
      const double res0n = -r.Ts * (cc.et.soc(0, 1) - cc.et.soc(0, 0)) / (3600 * r.Q);
      const double res0p = -r.Ts * (cc.et.soc(1, 1) - cc.et.soc(1, 0)) / (3600 * r.Q);
      const double dUn = cc.et.f(0, EF_DU, cc.et.soc(0, xSOC)), dUp = cc.et.f(1, EF_DU, cc.et.soc(1, xSOC));
      const double c0v[7] = {0.0, ChVz[NX], res0n, res0p, dUn * res0n, dUp * res0p, -dUn * res0n};
      auto chrow = [&](int q, double row[NA6]) {
#pragma unroll
        for (int k = 0; k < NX; ++k) {
          double a = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) a = a + xi.g[j] * cc.L[xi.m[j] * cc.stride + q * NX + k];
          if (rowf(r, q, G_PPHIS)) a = a + ChVz[k];
          row[k] = a;
        }
      };
      double ph0[NA6];
      chrow(R_PHISE0, ph0);
      double *zo = io.zbk + c * (nz + 2);
#pragma unroll 1
      for (int q = 0; q < nz; ++q) {
        double row[NA6];
        chrow(q, row);
        if (rowf(r, q, G_PHIE))
#pragma unroll
          for (int k = 0; k < NX; ++k) row[k] = row[k] - ph0[k];
        row[NX] = c0v[r.c0k[q]];
        zo[r.perm[q]] = 3 * sqrt(qform6(Sf, row));
      }
      zo[nz] = 3 * sqrt(qform6(Sf, ChVz));
      zo[nz + 1] = 3 * sqrt(rs * Sf[NA6 * NA6 - 1] * rs);
    }
    if (io.zk) {
#pragma unroll
      for (int q = 0; q < NZ; ++q)
        if (q < nz) io.zk[c * (nz + 2) + r.perm[q]] = Z[q];
      io.zk[c * (nz + 2) + nz] = vhat;
      io.zk[c * (nz + 2) + nz + 1] = Zsoc;
    }
    if (io.bnd) io.bnd[BD_M * s.n + c] = -1.0;  // no k_bounds record in MB
    if (io.xm_out) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { io.xm_out[c * 4 + j] = xi.m[j]; io.xg_out[c * 4 + j] = xi.g[j]; }
    }
    } else {
    double x0 = s.x0[c] + s.priorI[c];  // iterEKF.m:85-86 (models: k_bulk)
    double S0 = s.S0[c] + cf.SigmaW;
    const double SOC0 = s.SOC0[c];
    double SOC = SOC0 - x0 * (r.Ts / (3600 * r.Q));
    STAMP(1);
    get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC, xi);
    STAMP(2);
    // The 4 corner records are read once, whole (one round trip), advanced over the
    // steps their (deferred) time update skipped, used by getVariables and the gains,
    // updated and stored once; the updated xhat feeds the second getVariables and
    // EKFmatsHandler when the second getXind names the same corners.  A corner repeating
    // an earlier one (single-set-point grids) is a duplicate: the reference updates that
    // model twice in sequence, the second time from the state the first update left.
    const int t = io.lazy_t;
    bool dup[4];
    int tsj[4];
    double xr[4][NX], Sr[4][NPK];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dup[j] = false;
#pragma unroll
      for (int i = 0; i < j; ++i) dup[j] = dup[j] || xi.m[i] == xi.m[j];
    }
    // The corner window (KState::hot_*).  hot: this step's four records go to
    // the window's slots 0..3 (a cell with a repeated corner keeps the record path).  hit: slot j
    // already holds corner j's model for all four, so they are read from there as well.  A
    // lane whose tags differ from its corners in any position first writes every held slot back
    // to s.ekf / ts_ekf and reads its records there, as without a window (a model that moves
    // from one slot to another at a set-point crossing goes through its record).  The loads and
    // stores below are one code path: a per-lane base pointer and pair stride.
    const size_t hn = (size_t)s.n;
    const bool win = s.hot_m != nullptr && t != 0;
    bool hot = false, hit = false;
    if (win) {
      int hm[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) hm[j] = s.hot_m[j * hn + c];
      hot = !(dup[1] || dup[2] || dup[3]);
      hit = hot && hm[0] == xi.m[0] && hm[1] == xi.m[1] && hm[2] == xi.m[2] && hm[3] == xi.m[3];
      if (!hit) {
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
          const int mh = s.hot_m[j * hn + c];
          if (mh < 0) continue;
          double xh[NX], Sh[NPK];
          load_rec(hot_slot(s, j, c), xh, Sh, hn);
          store_rec(cc.erec + (size_t)mh * REC, xh, Sh);
          s.ts_ekf[c * r.NM + mh] = s.hot_ts[j * hn + c];
          if (!hot) s.hot_m[j * hn + c] = -1;
        }
      }
    }
    const size_t rst = hit ? hn : 1;  // pair stride of the four records' loads
    const size_t wst = hot ? hn : 1;  // and of their stores
    auto rrec = [&](int j) -> const double * { return hit ? hot_slot(s, j, c) : cc.erec + (size_t)xi.m[j] * REC; };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // corner 0's Sigma is what the gains use first: its whole record is read here; the
      // other corners read Sigma at their update (holding more spills: DESIGN.md 4.2)
      if (j == 0) load_rec(rrec(j), xr[j], Sr[j], rst);
      else load_x(rrec(j), xr[j], rst);
      const int *tp = hit ? s.hot_ts + j * hn + c : s.ts_ekf + c * r.NM + xi.m[j];
      tsj[j] = t ? *tp : 0;
    }
    // step t's ring input: the plant stores this cell's priorI there (k_plant4; cell_plant's
    // is stored only after body)
    const double pt = t ? (fplant ? s.priorI[c] : s.hist_p[(size_t)(t % LAZY_H) * s.n + c]) : 0.0;
    run_plant();
    if (planted) vk = vplant;
    if (t) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!dup[j]) replay_x(xr[j], cc.L + xi.m[j] * cc.stride + NZ * NX + NZ, tsj[j], t, pt, s, c);
#pragma unroll
      for (int j = 1; j < 4; ++j)
#pragma unroll
        for (int i = j - 1; i >= 0; --i)
          if (xi.m[i] == xi.m[j])
#pragma unroll
            for (int k = 0; k < NX; ++k) xr[j][k] = xr[i][k];
    }
    STAMP(3);
    KR kr1;
    vhat = get_vars<NZ>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xr, 0, &kr1);
    STAMP(4);
    if (st & ST_ERROR) {
      s.status[c] = st;
      s.warn[c] = warn;
      if (fused) s.uk[c] = NaN;
      fail_outputs();
      return;
    }
    __builtin_amdgcn_sched_barrier(0);
    double ChatV[4][NX], C0;
    get_chatv<NZ>(r, cc, xi, SOC0 - x0 * (r.Ts / (3600 * r.Q)), Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3], ChatV, C0,
                  &kr1);
    if (t) replay_S(Sr[0], cc.L + xi.m[0] * cc.stride + NZ * NX + NZ, tsj[0], t, cf.SigmaW);
    double St[4], Lg[4][NX];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double row[NX];
#pragma unroll
      for (int cI = 0; cI < NX; ++cI) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NX; ++k) acc = __builtin_fma(Sr[0][pk(k, cI)], ChatV[j][k], acc);
        row[cI] = acc;
      }
      double acc = 0.0;
#pragma unroll
      for (int cI = 0; cI < NX; ++cI) acc = __builtin_fma(row[cI], ChatV[j][cI], acc);
      St[j] = acc + cf.SigmaV;
#pragma unroll
      for (int k = 0; k < NX; ++k) Lg[j][k] = row[k] / St[j];
    }
    double St0 = C0 * S0 * C0 + cf.SigmaV;
    double L0 = S0 * C0 / St0;
    double res = vk - vhat;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      launder(St[j]);
#pragma unroll
      for (int k = 0; k < NX; ++k) launder(Lg[j][k]);
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(5);
    double xu[4][NX];  // corner j's xhat after its update
    // Corner j+1's Sigma is loaded before corner j's record is stored.  On
    // gfx950 one counter (vmcnt) covers loads and stores in issue order, so a load issued
    // after a store cannot be waited for without waiting for the store as well; loaded one
    // corner ahead, the wait for Sigma_{j+1} no longer includes corner j's store.  A corner
    // that repeats an earlier model (dup) reads its record after that store, as before.
    double Sn[NPK];
    auto s_ahead = [&](int j) { return j >= 1 && j < 4 && !dup[j]; };
    if (s_ahead(1)) load_S(rrec(1), Sn, rst);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double *rec = cc.erec + (size_t)xi.m[j] * REC;  // a repeated corner's (dup: never in the window)
      double xj[NX], Sj[NPK];
      if (dup[j]) {
        load_rec(rec, xj, Sj);  // as the earlier update of this model left it
      } else {
#pragma unroll
        for (int k = 0; k < NX; ++k) xj[k] = xr[j][k];
        if (j == 0) {
#pragma unroll
          for (int k = 0; k < NPK; ++k) Sj[k] = Sr[j][k];
        } else {  // loaded one corner ahead (s_ahead(j): j >= 1 and not a duplicate)
#pragma unroll
          for (int k = 0; k < NPK; ++k) Sj[k] = Sn[k];
        }
        if (t && j > 0) replay_S(Sj, cc.L + xi.m[j] * cc.stride + NZ * NX + NZ, tsj[j], t, cf.SigmaW);
      }
      meas_update_regs<false>(xj, Sj, Lg[j], St[j], res);
      if (j + 1 < 4 && s_ahead(j + 1)) load_S(rrec(j + 1), Sn, rst);
      // to window slot j with tag m[j] and timestamp t (a hit rewrites no tag and touches no
      // ts_ekf), or to the record
      store_rec(hot ? hot_slot(s, j, c) : rec, xj, Sj, wst);
      if (t) {
        *(hot ? s.hot_ts + j * hn + c : s.ts_ekf + c * r.NM + xi.m[j]) = t;
        if (hot && !hit) s.hot_m[j * hn + c] = xi.m[j];
      }
#pragma unroll
      for (int k = 0; k < NX; ++k) xu[j][k] = xj[k];
      __builtin_amdgcn_sched_barrier(0);
    }
    STAMP(6);
    x0 = __builtin_fma(L0, res, x0);
    S0 = S0 - L0 * St0 * L0;
    SOC = SOC0 - x0 * (r.Ts / (3600 * r.Q));
    int m1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m1[j] = xi.m[j];
    get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC, xi);
    // same corners: their xhat is in registers and current; else catch the new corners
    // up and read them (their records are the stored ones)
    const bool same = m1[0] == xi.m[0] && m1[1] == xi.m[1] && m1[2] == xi.m[2] && m1[3] == xi.m[3] &&
                      !(dup[1] || dup[2] || dup[3]);
    if (!same) {
      // with the window, a corner that is one of the four just updated is current only there
      // and in xu: it is taken from xu and never re-read from s.ekf; a new model is not in
      // the window (its slots hold exactly m1) and goes through its record, as without one
      bool held[4];
      double xn[4][NX];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        held[j] = false;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (hot && m1[i] == xi.m[j]) {
            held[j] = true;
#pragma unroll
            for (int k = 0; k < NX; ++k) xn[j][k] = xu[i][k];
          }
      }
      if (io.lazy_t) ekf_catch_up4<NZ>(s, cc, r.NM, xi.m, c, io.lazy_t, cf.SigmaW, pt, held);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!held[j]) load_x(cc.erec + (size_t)xi.m[j] * REC, xn[j]);
#pragma unroll
        for (int k = 0; k < NX; ++k) xu[j][k] = xn[j][k];
      }
    }
    STAMP(7);
    vhat = get_vars<NZ>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xu, 0, &kr2);
    have_kr2 = true;
    const int jm = corner_max(xi);
#pragma unroll
    for (int k = 0; k < NX; ++k) xmax[k] = jm == 0 ? xu[0][k] : jm == 1 ? xu[1][k] : jm == 2 ? xu[2][k] : xu[3][k];
    have_xmax = true;
    __builtin_amdgcn_sched_barrier(0);
    STAMP(8);
    s.warn[c] = warn;
    if (st & ST_ERROR) {
      s.status[c] = st;
      s.x0[c] = x0;
      s.S0[c] = S0;
      if (fused) s.uk[c] = NaN;
      fail_outputs();
      return;
    }
    if (io.bnd) {  // boundzk (iterEKF.m:186-205) runs in k_bounds from this record
      double *bd = io.bnd;
      const int64_t n = s.n;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bd[(BD_G + j) * n + c] = xi.g[j];
        bd[(BD_M + j) * n + c] = xi.m[j];
      }
      const BoundK b =
          bound_k(r, cc, SOC0 - x0 * (r.Ts / (3600 * r.Q)), Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3], &kr2);
#pragma unroll
      for (int i = 0; i < 11; ++i) bd[(BD_K + i) * n + c] = bound_field(b, i);
      bd[BD_S0 * n + c] = S0;
    }
    STAMP(9);
    s.x0[c] = x0;
    s.S0[c] = S0;
    s.priorI[c] = ik;  // iterEKF.m:210
    if (io.zk) {
#pragma unroll
      for (int q = 0; q < NZ; ++q)
        if (q < nz) io.zk[c * (nz + 2) + r.perm[q]] = Z[q];
      io.zk[c * (nz + 2) + nz] = vhat;
      io.zk[c * (nz + 2) + nz + 1] = Zsoc;
    }
    if (io.xm_out) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { io.xm_out[c * 4 + j] = xi.m[j]; io.xg_out[c * 4 + j] = xi.g[j]; }
    }
    }  // OB
  }
  if (!(PARTS & (P_MPC | P_LIN))) return;
  // The fused step's second kernel: cells the iterEKF kernel failed are finished.
  if (!(PARTS & P_EKF) && fused) {
    if (st & ST_ERROR) return;
    vk = s.vk[c];
  }

  Lin L;
  if (io.mode & (MODE_LIN | MODE_FUSED)) {
    double zr[NROLE];
    if (fused && (PARTS & P_EKF)) {
#pragma unroll
      for (int q = 0; q < NROLE; ++q) zr[q] = Z[q];
    } else {
      if (!fused && (st & ST_ERROR)) { fail_outputs(); return; }
#pragma unroll
      for (int q = 0; q < NROLE; ++q) zr[q] = io.zk_in[c * (nz + 2) + r.perm[q]];
      Zsoc = io.zk_in[c * (nz + 2) + nz + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) { xi.m[j] = io.xm_in[c * 4 + j]; xi.g[j] = io.xg_in[c * 4 + j]; }
    }
    if constexpr (!(PARTS & P_EKF) && !MB) {
      // the fused step's second kernel: EKFmatsHandler's corner may be held in the corner
      // window, where the iterEKF kernel left it (its s.ekf record is then stale)
      if (fused && s.hot_m && io.lazy_t) {
        int mx;
        (void)corner_max(xi, &mx);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!have_xmax && s.hot_m[(size_t)j * s.n + c] == mx) {
            load_x(hot_slot(s, j, c), xmax, (size_t)s.n);
            have_xmax = true;
          }
      }
    }
    mats_handler<NZ>(r, cc, xi, zr, Zsoc, Tc + 273.15, L, MB ? s.x0[c] : 0.0, xmax, fused && have_xmax,
                     fused && (PARTS & P_EKF) && have_kr2 ? &kr2 : nullptr);
    if (io.lin_out) lin_store(io.lin_out + c * 35, L);
    if (io.x_out)
#pragma unroll
      for (int q = 0; q < 6; ++q) io.x_out[c * 6 + q] = L.xhat[q];  // x_store (runMPC.m:108)
  }
  STAMP(10);
  if (PARTS & P_LIN) {  // iterMPC runs in the wide-horizon kernels (mpcekf_wide.hip) from lin_out / zsoc_out
    if (fused) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = acc + L.Cphi[k] * L.xhat[k];
      if (io.phise) io.phise[c] = acc + s.uk[c] * L.Dphi + L.bphi;  // runMPC.m:94-95
      if (io.v) io.v[c] = vk;
      if (io.soc) io.soc[c] = Zsoc;
      if (io.zsoc_out) io.zsoc_out[c] = Zsoc;
    }
    return;
  }

  if (io.mode & (MODE_MPC | MODE_FUSED)) {
    if (!fused) {
      if (st & ST_ERROR) { fail_outputs(); return; }
      lin_load(io.lin_in + c * 35, L);
      Zsoc = io.soc_k1_in[c];
    }
    double uk_1 = s.uk_1[c];
    double ukin = fused ? s.uk[c] : 0.0;
    double phise = 0.0;
    if (fused) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = acc + L.Cphi[k] * L.xhat[k];
      phise = acc + ukin * L.Dphi + L.bphi;  // runMPC.m:94-95
    }
    MpcOut o;
    MpcSetup Pm;
    bool need = mpc_setup(cf, L, uk_1, Zsoc, Pm, o);
    if (fused) {
      if (io.v) io.v[c] = vk;
      if (io.soc) io.soc[c] = Zsoc;
      if (io.phise) io.phise[c] = phise;
    }
    if (s.J_unc) s.J_unc[c] = o.J_unc;
    if (io.junc_out) io.junc_out[c] = o.J_unc;
    STAMP(11);
    s.hflag[c] = need ? 1 : 0;
    if (need) {  // hildreth.m runs in k_hild
      double *pb = s.prob;
      const int64_t n = s.n;
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        pb[(PB_F + a) * n + c] = Pm.F[a];
#pragma unroll
        for (int b = 0; b < NC; ++b) pb[(PB_E + a * NC + b) * n + c] = Pm.E[a][b];
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        pb[(PB_HV + i) * n + c] = Pm.Cn.Hv[i];
        pb[(PB_HE + i) * n + c] = Pm.Cn.He[i];
        pb[(PB_HS + i) * n + c] = Pm.Cn.Hs[i];
        pb[(PB_ERR + i) * n + c] = Pm.e[i];
      }
#pragma unroll
      for (int i = 0; i < NCON; ++i) pb[(PB_GAM + i) * n + c] = Pm.Cn.gam[i];
      pb[PB_RU * n + c] = Pm.Ru;
      pb[PB_UK1 * n + c] = uk_1;
    } else {
      o.nexec = 0;
      mpc_finish(Pm.Cn, Pm.e, Pm.Ru, Pm.DU, uk_1, o);
      s.uk_1[c] = uk_1;
      if (s.J_fin) { s.J_fin[c] = o.J_fin; s.nviol[c] = o.nviol; }
      cost_out(io, c, o.J_fin, o.nviol, norm_du<NC>(Pm.DU));
      if (io.uk_out) io.uk_out[c] = o.uk;
      if (io.nexec) io.nexec[c] = 0;
      if (fused) {
        s.uk[c] = o.uk;
        if (io.u) io.u[c] = o.uk;
      }
    }
  }
  };
  body();
  if (ring_late) {  // every path of body ran the plant; the ring's slot t is read by no load of this step
    const size_t slot = (size_t)(io.lazy_t % LAZY_H) * s.n + c;
    s.hist_u[slot] = ring_u;
    s.hist_p[slot] = ring_p;
  }
}

// OB_step's simStep (OB_step.m:188-357) at the start of k_ekf4's fused step: k_plant4's lane
// quad (lane j = corner j: its gather, replay and 9 output rows; the blend by quad
// broadcasts in the one-lane order; the per-cell scalar chain the same in all four lanes)
// on cell_plant's cell-blob layout.  Every live lane stores the per-cell values (the same
// bits), so each lane's later reads of them (the ring slot of this step) follow its own
// store.  Returns Vcell in every lane of the quad: the shared plant helpers' expressions,
// hence k_plant4's and cell_plant's bits.
template <int NZ, bool PL>
__device__ __forceinline__ double quad_plant(const KRom &r, const KState &s, const double *L, const double *tb,
                                             const double *Tp, const double *Zp, int64_t c, int j, bool live,
                                             int lazy_t, double Iapp, double tcs, int st) {
  constexpr int OA = NZ * NX + NZ, OR0 = NZ * NX + NZ + NX + NPK, OD = NZ * NX;
  const int stride = r.cell_stride;
  if (lazy_t && live) {  // this step's inputs, for the deferred updates of every model
    const size_t slot = (size_t)(lazy_t % LAZY_H) * s.n + c;
    s.hist_u[slot] = Iapp;
    s.hist_p[slot] = s.priorI[c];
  }
  if (st & ST_ERROR) return __builtin_nan("");
  const double T = tcs + 273.15;  // OB_step.m:75
  const ETab et = etab<PL>(r, tb + r.cell_tab, T);
  double SOCnAvg = s.SOCn[c], SOCpAvg = s.SOCp[c];
  const double SOC0n = s.SOC0n[c], SOC0p = s.SOC0p[c];
  const double negSOC = SOCnAvg, posSOC = SOCpAvg;  // obs.negSOC / posSOC: pre-update (OB_step.m:226-227)
  double cellSOC = (SOCnAvg - r.th0n) / (r.th100n - r.th0n);
  const PlantCorners pc = plant_corners(r, Tp, Zp, cellSOC, T);
  const int mj = corner_model(r, pc, j);  // this lane's corner
  double *bx = s.bigx + ((size_t)c * r.NM + mj) * 6;
  double xs[6];
  load_corner(bx, xs);
  const int tsj = lazy_t ? s.ts_plant[c * r.NM + mj] : 0;
  plant_soc_step(r, et, SOC0n, SOC0p, Iapp, SOCnAvg, SOCpAvg);
  double aZ, aT;
  plant_weights(Tp, Zp, pc, cellSOC, T, aZ, aT);
  const double *a = L + mj * stride + OA;
  if (lazy_t) plant_replay<false>(xs, a, s, c, tsj, lazy_t);
  const double *B = L + mj * stride;
  double yk[NPLANT];
#pragma unroll
  for (int q = 0; q < NPLANT; ++q)
    yk[q] = quad_blend(plant_row(B + q * NX, B[OR0 + q], B[OD + q], xs, Iapp), aZ, aT);
  const double V = plant_vcell(r, et, yk, T, Iapp, negSOC, posSOC, SOC0n, SOC0p);
  if (live) {
    s.SOCn[c] = SOCnAvg;
    s.SOCp[c] = SOCpAvg;
  }
  if (live && lazy_t && tsj < lazy_t) {  // advance this corner through step t in place
    double x[6];
    plant_advance<false>(a, xs, Iapp, x);
    store_corner(bx, x);
    s.ts_plant[c * r.NM + mj] = lazy_t;
  }
  return V;
}

// ---------------------------------------------------------------------------
// k_ekf4: the fused step's iterEKF ('OB', iterEKF.m:55-210) with a lane quad per cell,
// lane j = corner j of getXind: its record's catch-up, its getVariables term, its
// getChatV row, gain and measurement update run in parallel; the corner sums keep the
// one-lane order through DPP broadcasts (get_vars<NZ, true>), so every result is
// k_cell's to the bit.  EKFmatsHandler + iterMPC follow in k_cell<NZ, P_MPC> from the
// zk / Xind hand-off.  Needs distinct corners (nT > 1 and nZ > 1; host checks).
// 1024-thread blocks (256 cells): the ~130 KB ROM blob is staged once per CU and the
// CU runs 4 waves per SIMD.
// ---------------------------------------------------------------------------
template <int NZ, int BLOCK, bool GR, bool PL>
__global__ void __launch_bounds__(BLOCK) k_ekf4(const KRom r, const KCfg cf, const KState s, const KIO io) {
  extern __shared__ double lds[];
  const int lo = GR ? r.cell_tab : 0;  // GR: model rows from the global blob (k_plant4)
  stage_lds(lds, r.cell_blob + lo, r.cell_len - lo);
  __syncthreads();
  const double *tb = lds - lo;
  const double *Tp = tb + r.cell_tab + r.cell_tablen;
  const double *Zp = Tp + MAXT;
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = s.n;
  const int j = (int)(gt & 3);
  const int64_t cq = gt >> 2;
  const bool live = cq < n;
  const int64_t c = live ? cq : n - 1;  // lanes past n ride along (quad exchanges), write nothing
  const int nz = r.nz;
  const double NaN = __builtin_nan("");
  CellCtx cc;
  cc.L = GR ? r.cell_blob : lds;
  cc.Tp = Tp;
  cc.Zp = Zp;
  cc.erec = s.ekf + (size_t)c * r.NM * REC;
  cc.stride = r.cell_stride;
  const bool fplant = io.plant;  // OB_step's simStep runs here (KRom::cell_plant; k_cell's fplant)
  const double Tc = fplant && io.tc_in ? io.tc_in[c] : s.Tc[c];
  if (fplant && io.tc_in && live && j == 0) s.Tc[c] = Tc;  // this step's TC (runMPC.m:85-92)
  cc.T = Tc > 100 ? Tc : Tc + 273.15;  // iterEKF.m:62-66
  cc.et = etab<PL>(r, tb + r.cell_tab, cc.T);
  int st = s.status[c];
  const int t = io.lazy_t;
  if (live && j == 0) s.hflag[c] = 0;
  // runMPC.m:85: [voltage, ...] = OB_step(uk, TC, cellState, ROM) first
  double vplant = 0.0;
  if (fplant) {
    if (gt == 0 && t) *s.hslow = 0;  // k_hild_slow of the previous step has finished
    vplant = quad_plant<NZ, PL>(r, s, cc.L, tb, Tp, Zp, c, j, live, t, s.uk[c], Tc, st);
    if (live && j == 0) s.vk[c] = vplant;
  }
  auto fail_outputs = [&]() {
    if (!live) return;
    if (j == 0) {
      if (io.u) io.u[c] = NaN;
      if (io.v) io.v[c] = NaN;
      if (io.soc) io.soc[c] = NaN;
      if (io.phise) io.phise[c] = NaN;
      if (io.nexec) io.nexec[c] = 0;
      if (io.bnd) io.bnd[BD_M * n + c] = -1.0;
      if (io.x_out)
        for (int q = 0; q < 6; ++q) io.x_out[c * 6 + q] = NaN;
      if (io.junc_out) io.junc_out[c] = NaN;
      if (io.jfin_out) io.jfin_out[c] = NaN;
      if (io.normdu_out) io.normdu_out[c] = NaN;
      if (io.nviol_out) io.nviol_out[c] = 0;
    }
    if (io.zk)
      for (int q = j; q < nz + 2; q += 4) io.zk[c * (nz + 2) + q] = NaN;
    if (io.zbk)
      for (int q = j; q < nz + 2; q += 4) io.zbk[c * (nz + 2) + q] = NaN;
    if (io.xm_out) { io.xm_out[c * 4 + j] = -1; io.xg_out[c * 4 + j] = NaN; }
  };
  if (st & ST_ERROR) {
    fail_outputs();
    return;
  }
  const double ik = s.uk[c], vk = fplant ? vplant : s.vk[c];
  int warn = s.warn[c];
  if (warn > cf.max_warn) {  // iterEKF.m:55-59
    st |= ST_LOCKOUT | ST_ERROR;
    if (live && j == 0) { s.status[c] = st; s.uk[c] = NaN; }
    fail_outputs();
    return;
  }
  double x0 = s.x0[c] + s.priorI[c];  // iterEKF.m:85-86
  double S0 = s.S0[c] + cf.SigmaW;
  const double SOC0 = s.SOC0[c];
  XI xi;
  get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC0 - x0 * (r.Ts / (3600 * r.Q)), xi);
  // this lane's corner: record, caught up over the steps its time update skipped
  const int mj = xi.m[j];
  double *rec = cc.erec + (size_t)mj * REC;
  const double *am = cc.L + mj * cc.stride + NZ * NX + NZ;  // diag(A), then a_p a_q
  double xr[1][NX];
  load_x(rec, xr[0]);
  const int tsj = s.ts_ekf[c * r.NM + mj];
  const double pt = s.hist_p[(size_t)(t % LAZY_H) * n + c];
  replay_x(xr[0], am, tsj, t, pt, s, c);
  __builtin_amdgcn_sched_barrier(0);
  double Z[NZ], Zsoc;
  double vhat = get_vars<NZ, true>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xr, j);
  if (st & ST_ERROR) {
    if (live && j == 0) { s.status[c] = st; s.warn[c] = warn; s.uk[c] = NaN; }
    fail_outputs();
    return;
  }
  __builtin_amdgcn_sched_barrier(0);
  // getChatV (iterEKF.m:421-519): this corner's row; gains against corner 1's Sigma
  const ChatK K = chat_k(r, cc, SOC0 - x0 * (r.Ts / (3600 * r.Q)), Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3]);
  double Ch[NX];
  chat_row(r, K, cc.L + mj * cc.stride, xi.g[j], Ch);
  const double C0 = chat0(r, K);
  double Sj[NPK];
  load_S(rec, Sj);
  replay_S(Sj, am, tsj, t, cf.SigmaW);
  double S1[NPK];
#pragma unroll
  for (int i = 0; i < NPK; ++i) S1[i] = qbc<0>(Sj[i]);
  double row[NX];
#pragma unroll
  for (int cI = 0; cI < NX; ++cI) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NX; ++k) acc = __builtin_fma(S1[pk(k, cI)], Ch[k], acc);
    row[cI] = acc;
  }
  double acc = 0.0;
#pragma unroll
  for (int cI = 0; cI < NX; ++cI) acc = __builtin_fma(row[cI], Ch[cI], acc);
  const double Stj = acc + cf.SigmaV;
  double Lg[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) Lg[k] = row[k] / Stj;
  const double St0 = C0 * S0 * C0 + cf.SigmaV;
  const double L0 = S0 * C0 / St0;
  const double res = vk - vhat;
  __builtin_amdgcn_sched_barrier(0);
  // iterEKF.m:137-153: corner j's record (distinct corners: the updates are independent)
  meas_update_regs<true>(xr[0], Sj, Lg, Stj, res);
  if (live) {
    store_rec(rec, xr[0], Sj);
    s.ts_ekf[c * r.NM + mj] = t;
  }
  __builtin_amdgcn_sched_barrier(0);
  x0 = __builtin_fma(L0, res, x0);
  S0 = S0 - L0 * St0 * L0;
  int mold[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) mold[i] = xi.m[i];
  get_xind(r.nT, r.nZ, Tp, Zp, cc.T, SOC0 - x0 * (r.Ts / (3600 * r.Q)), xi);
  // the new corner j: one this step just updated (its state comes from that lane's
  // registers), or an untouched model whose record is caught up to step t here
  // (ekf_catch_up4)
  const int mn = xi.m[j];
  int src = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (mold[i] == mn) src = i;
  {
    const int from = (threadIdx.x & ~3) + (src < 0 ? j : src);
#pragma unroll
    for (int k = 0; k < NX; ++k) xr[0][k] = shfl64(xr[0][k], from);
  }
  if (src < 0) {
    double *recn = cc.erec + (size_t)mn * REC;
    const int tsn = s.ts_ekf[c * r.NM + mn];
    double Sn[NPK];
    load_rec(recn, xr[0], Sn);
    if (tsn < t) {
      const double *an = cc.L + mn * cc.stride + NZ * NX + NZ;
      replay_x(xr[0], an, tsn, t, pt, s, c);
      replay_S(Sn, an, tsn, t, cf.SigmaW);
      if (live) {
        store_rec(recn, xr[0], Sn);
        s.ts_ekf[c * r.NM + mn] = t;
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  vhat = get_vars<NZ, true>(r, cc, xi, ik, x0, SOC0, warn, st, Z, Zsoc, xr, j);
  __builtin_amdgcn_sched_barrier(0);
  if (!live) return;
  if (j == 0) s.warn[c] = warn;
  if (st & ST_ERROR) {
    if (j == 0) { s.status[c] = st; s.x0[c] = x0; s.S0[c] = S0; s.uk[c] = NaN; }
    fail_outputs();
    return;
  }
  if (io.bnd) {  // boundzk (iterEKF.m:186-205) runs in k_bounds from this record
    io.bnd[(BD_G + j) * n + c] = xi.g[j];
    io.bnd[(BD_M + j) * n + c] = xi.m[j];
    const BoundK b = bound_k(r, cc, SOC0 - x0 * (r.Ts / (3600 * r.Q)), Z[R_TE1], Z[R_TH0], Z[R_TEE], Z[R_TH3]);
#pragma unroll
    for (int i = 0; i < 11; ++i)
      if ((i & 3) == j) io.bnd[(BD_K + i) * n + c] = bound_field(b, i);
    if (j == 3) io.bnd[BD_S0 * n + c] = S0;
  }
  if (j == 0) {
    s.x0[c] = x0;
    s.S0[c] = S0;
    s.priorI[c] = ik;  // iterEKF.m:210
  }
  if (io.zk) {
#pragma unroll
    for (int q = 0; q < NZ; ++q)
      if (q < nz && (q & 3) == j) io.zk[c * (nz + 2) + r.perm[q]] = Z[q];
    if (j == 1) io.zk[c * (nz + 2) + nz] = vhat;
    if (j == 2) io.zk[c * (nz + 2) + nz + 1] = Zsoc;
  }
  if (io.xm_out) { io.xm_out[c * 4 + j] = xi.m[j]; io.xg_out[c * 4 + j] = xi.g[j]; }
}

// ---------------------------------------------------------------------------
// k_bounds: boundzk (iterEKF.m:186-205; getChatZ iterEKF.m:523-602), diagonal only.
// A lane quad per cell, lane j = corner j: its getChatV row, its 26 quadratic forms
// row' * Sigma1 * row; the corner sums keep k_cell's order ((((0 + q0) + q1) + q2)
// + q3) through DPP broadcasts, so the result is the one-lane form's bits.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double quad_sum_seq(double v) {  // (((0 + v0) + v1) + v2) + v3
  return (((0.0 + qbc<0>(v)) + qbc<1>(v)) + qbc<2>(v)) + qbc<3>(v);
}

// 256 cells per block: the ~90 KB model blob leaves room for one block per CU, so the
// block is the CU's whole occupancy (4 waves per SIMD) and stages the blob once.
constexpr int BOUNDS_BLOCK = 1024;
// k_bounds stages only the models of the cell blob (its getChatV scalars come from k_cell)
__host__ __device__ inline int bounds_c0_base(const KRom &r) { return r.rom_global ? 0 : r.cell_tab + 1; }
template <int NZ, bool GR>
__global__ void __launch_bounds__(BOUNDS_BLOCK) k_bounds(const KRom r, const KState s, const double *bd, double *zbk) {
  extern __shared__ double lds[];
  if (!GR) stage_lds(lds, r.cell_blob, r.cell_tab);  // GR: model rows from the global blob
  __syncthreads();
  const double *L = GR ? r.cell_blob : lds;
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = s.n;
  const int j = (int)(gt & 3);
  const int64_t cq = gt >> 2;
  const int64_t c = cq < n ? cq : n - 1;  // lanes past n ride along (quad exchanges)
  const int nz = r.nz;
  const bool valid = cq < n && bd[BD_M * n + c] >= 0.0;
  const double g = bd[(BD_G + j) * n + c];
  const int m = valid ? (int)bd[(BD_M + j) * n + c] : 0;
  const double *Cm = L + m * r.cell_stride;
  const double S0 = bd[BD_S0 * n + c];
  // SigmaX of the first corner for all four (iterEKF.m:191)
  double S1b[NPK];
  // from the corner window when a slot holds that model (the usual case: k_cell has just
  // stored it there, and the read is coalesced across the wave's cells), else from its record
  const int m0 = valid ? (int)bd[BD_M * n + c] : 0;
  int hslot = -1;
  if (s.hot_m) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (valid && s.hot_m[(size_t)i * n + c] == m0) hslot = i;
  }
  load_S(hslot >= 0 ? hot_slot(s, hslot, c) : s.ekf + ((size_t)c * r.NM + m0) * REC, S1b, hslot >= 0 ? (size_t)n : 1);
#pragma unroll
  for (int k = 0; k < NX; ++k)
#pragma unroll
    for (int l = k + 1; l < NX; ++l) S1b[pk(k, l)] = 2 * S1b[pk(k, l)];
  // getChatV's scalars at the updated state, from k_cell (bound_k)
  ChatK K;
  K.Rfn = bd[(BD_K + 0) * n + c];
  K.Rfp = bd[(BD_K + 1) * n + c];
  K.Rctn = bd[(BD_K + 2) * n + c];
  K.Rctp = bd[(BD_K + 3) * n + c];
  K.dUn0 = bd[(BD_K + 4) * n + c];
  K.dUp3 = bd[(BD_K + 5) * n + c];
  double ChV[NX];
  chat_row(r, K, Cm, g, ChV);
  const double ChV0 = bd[BD_C0 * n + c];
  const double res0n = bd[BD_R0N * n + c], res0p = bd[BD_R0P * n + c];
  const double dUn = bd[BD_DUN * n + c], dUp = bd[BD_DUP * n + c];
  const bool ph0pp = rowf(r, R_PHISE0, G_PPHIS);
  double cph0[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    double v = g * Cm[R_PHISE0 * NX + k];
    if (ph0pp) v = v + ChV[k];
    cph0[k] = v;
  }
  // The constant-column terms (c0 * S0) * c0 of the 7 kinds (C0_*) in an LDS row per
  // cell, lane j filling kinds j and j + 4: each form then adds its term by a uniform
  // offset instead of a select chain.
  double *c0t = lds + (GR ? 0 : r.cell_tab + 1) + (threadIdx.x >> 2) * 8;
  {
    const double cv[8] = {0.0, ChV0, res0n, res0p, dUn * res0n, dUp * res0p, -dUn * res0n, 0.0};
    double lo = cv[0], hi = cv[4];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (j == i) { lo = cv[i]; hi = cv[i + 4]; }
    c0t[j] = (lo * S0) * lo;
    c0t[j + 4] = (hi * S0) * hi;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // Forms q = j, j + 4, ... are this lane's to finish: their sums and output slots.
  constexpr int NOWN = (NZ + 3) / 4;
  double mine[NOWN];
  int slot[NOWN];
#pragma unroll
  for (int i = 0; i < NOWN; ++i) { mine[i] = 0.0; slot[i] = -1; }
#pragma unroll
  for (int q = 0; q < NZ; ++q) {
    double row[NX];
    const bool fpp = rowf(r, q, G_PPHIS), fph = rowf(r, q, G_PHIE);
    // uniform branches (the empty volatile asm keeps them from being if-converted)
    if (fpp) {
      asm volatile("");
#pragma unroll
      for (int k = 0; k < NX; ++k) row[k] = __builtin_fma(g, Cm[q * NX + k], ChV[k]);
    } else {
      asm volatile("");
#pragma unroll
      for (int k = 0; k < NX; ++k) row[k] = g * Cm[q * NX + k];
    }
    if (fph) {
      asm volatile("");
#pragma unroll
      for (int k = 0; k < NX; ++k) row[k] = row[k] - cph0[k];
    }
    const double qf = qform(S1b, row);
    const double sz = quad_sum_seq(qf) + c0t[r.c0k[q]];
    if ((q & 3) == j && q < nz) {
      mine[q >> 2] = sz;
      slot[q >> 2] = r.perm[q];
    }
    __builtin_amdgcn_sched_barrier(0);  // one form at a time: 128 VGPRs at 4 waves/SIMD
  }
  double *zo = zbk + c * (nz + 2);
#pragma unroll
  for (int i = 0; i < NOWN; ++i)
    if (valid && slot[i] >= 0) zo[slot[i]] = 3 * sqrt(mine[i]);
  const double acc = qform(S1b, ChV);
  double SigV = quad_sum_seq(acc);
  SigV = SigV + ChV0 * S0 * ChV0;
  const double rr = -r.Ts / (3600 * r.Q);
  const double SigSOC = rr * S0 * rr;
  if (valid && j == 0) {
    zo[nz] = 3 * sqrt(SigV);
    zo[nz + 1] = 3 * sqrt(SigSOC);
  }
}

__global__ void __launch_bounds__(256) k_hild(const KCfg cf, const KState s, const KIO io) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= s.n) return;
  hild_cell(cf, s, io, c);
}

// The exact-rule solve of the cells k_hild flagged (hflag 2): one wave per block over a
// grid-stride range of waves, gone at once when k_hild counted none.
__global__ void __launch_bounds__(64) k_hild_slow(const KCfg cf, const KState s, const KIO io) {
  if (__builtin_amdgcn_readfirstlane(*s.hslow) == 0) return;
  for (int64_t w = blockIdx.x; w * 64 < s.n; w += gridDim.x) hild_slow_cell(cf, s, io, w * 64 + threadIdx.x);
}

// ---------------------------------------------------------------------------
// context-free batched kernels
// ---------------------------------------------------------------------------
__global__ void k_predmat(int64_t n, const double *a, const double *C, const double *D, double *Phi, double *G) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double av[6], Cb[7], P[NP][NA], H[NP];
#pragma unroll
  for (int k = 0; k < 6; ++k) { av[k] = a[c * 6 + k]; Cb[k] = C[c * 6 + k]; }
  Cb[6] = D[c];
  predmat_s(av, Cb, P, H);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
#pragma unroll
    for (int k = 0; k < NA; ++k) Phi[(c * NP + i) * NA + k] = P[i][k];
#pragma unroll
    for (int j = 0; j < NC; ++j) G[(c * NP + i) * NC + j] = j <= i ? H[i - j] : 0.0;
  }
}

__global__ void __launch_bounds__(64) k_constraints(const KCfg cf, int64_t n, const double *lin,
                                                    const double *uk_1, const double *soc_k1, double *Mo,
                                                    double *go) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  Lin L;
  lin_load(lin + c * 35, L);
  double dx[NA];
#pragma unroll
  for (int k = 0; k < 6; ++k) dx[k] = L.xhat[k];
  dx[6] = uk_1[c];
  double Phis[NP][NA], Hs[NP], Cb[7];
#pragma unroll
  for (int k = 0; k < 6; ++k) Cb[k] = L.Csoc[k];
  Cb[6] = L.Dsoc;
  predmat_s(L.a, Cb, Phis, Hs);
  Cons Cn;
  constraints_s(cf, L, dx, uk_1[c], soc_k1[c], Phis, Hs, Cn);
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    go[c * NCON + i] = Cn.gam[i];
#pragma unroll
    for (int j = 0; j < NC; ++j) Mo[(c * NCON + i) * NC + j] = mval(Cn, i, j);
  }
}

// hildreth.m for an arbitrary (E, F, M, gamma): M is data, not the pattern.
__global__ void __launch_bounds__(64) k_hildreth(int64_t n, const double *Ei, const double *Fi, const double *Mi,
                                                 const double *gi, double *lami, int maxIter, double tol,
                                                 double *DUo, int *nexec) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double E[NC][NC], F[NC], M[NCON][NC], gam[NCON], lam[NCON], DU[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    F[a] = Fi[c * NC + a];
#pragma unroll
    for (int b = 0; b < NC; ++b) E[a][b] = Ei[(c * NC + a) * NC + b];
  }
#pragma unroll
  for (int i = 0; i < NCON; ++i) {
    gam[i] = gi[c * NCON + i];
    lam[i] = lami[c * NCON + i];
#pragma unroll
    for (int j = 0; j < NC; ++j) M[i][j] = Mi[(c * NCON + i) * NC + j];
  }
  DenseM Mf{M};
  int it = hildreth_core(Mf, E, F, gam, lam, maxIter, tol, DU);
#pragma unroll
  for (int i = 0; i < NCON; ++i) lami[c * NCON + i] = lam[i];
#pragma unroll
  for (int a = 0; a < NC; ++a) DUo[c * NC + a] = DU[a];
  nexec[c] = it;
}

// hildreth.m for any Nc <= HANY_NC and nC <= HANY_NCON with a dense M (mpcekf_hildreth at
// sizes other than the fused Np = 5 / Nc = 2): orc_hildreth's defined evaluation with
// runtime sizes, lane per problem.  X = E\M' (Cholesky, else LU), H_ii and K live in a
// per-problem scratch slab; the dense path re-forms H(i,j) entry by entry.  A stage entry
// point, not the fused path: sized for correctness, not speed.
constexpr int HANY_NC = 10, HANY_NCON = 100;
__device__ inline bool chol_rt(int n, const double *E, double *R) {
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    double s = E[j * n + j];
    for (int k = 0; k < j; ++k) s = s - R[k * n + j] * R[k * n + j];
    if (!(s > 0)) ok = false;
    R[j * n + j] = sqrt(s);
    for (int i = j + 1; i < n; ++i) {
      double t = E[j * n + i];
      for (int k = 0; k < j; ++k) t = t - R[k * n + j] * R[k * n + i];
      R[j * n + i] = t / R[j * n + j];
    }
  }
  return ok;
}
__device__ inline void lu_rt(int n, const double *Ain, const double *b, double *x) {
  double A[HANY_NC * HANY_NC], y[HANY_NC];
  for (int i = 0; i < n * n; ++i) A[i] = Ain[i];
  for (int i = 0; i < n; ++i) y[i] = b[i];
  for (int k = 0; k < n; ++k) {
    int p = k;
    for (int i = k + 1; i < n; ++i)
      if (fabs(A[i * n + k]) > fabs(A[p * n + k])) p = i;
    if (p != k) {
      for (int j = 0; j < n; ++j) { const double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
      const double t = y[k]; y[k] = y[p]; y[p] = t;
    }
    for (int i = k + 1; i < n; ++i) {
      const double l = A[i * n + k] / A[k * n + k];
      A[i * n + k] = l;
      for (int j = k + 1; j < n; ++j) A[i * n + j] = A[i * n + j] - l * A[k * n + j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < i; ++k) y[i] = y[i] - A[i * n + k] * y[k];
  for (int i = n - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < n; ++k) t = t - A[i * n + k] * x[k];
    x[i] = t / A[i * n + i];
  }
}
// MATLAB E\b for symmetric E: Cholesky when every pivot is positive, else LU
__device__ inline void mldiv_rt(int n, const double *E, const double *R, bool ok, const double *b, double *x) {
  if (!ok) {
    lu_rt(n, E, b, x);
    return;
  }
  double y[HANY_NC];
  for (int i = 0; i < n; ++i) {
    double t = b[i];
    for (int k = 0; k < i; ++k) t = t - R[k * n + i] * y[k];
    y[i] = t / R[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < n; ++k) t = t - R[i * n + k] * x[k];
    x[i] = t / R[i * n + i];
  }
}
// t_i = K_i + M(i,:)*v (orc hild_row_t): Nc <= 2 fma in ascending k; else the 8-lane
// form: a_0 = fma(M_i0, v_0, K_i), a_k = M_ik v_k (+0 past Nc), b_k = fma(M_i,k+8, v_k+8, a_k)
// while k + 8 < Nc, then the pairwise tree over the 8 slots
__device__ inline double row_t_rt(int Nc, const double *Mi, const double *v, double Ki) {
  if (Nc <= 2) {
    double t = Ki;
    for (int k = 0; k < Nc; ++k) t = __builtin_fma(Mi[k], v[k], t);
    return t;
  }
  double b[8];
  for (int k = 0; k < 8; ++k) {
    const double a = k == 0 ? __builtin_fma(Mi[0], v[0], Ki) : (k < Nc ? Mi[k] * v[k] : 0.0);
    b[k] = k + 8 < Nc ? __builtin_fma(Mi[k + 8], v[k + 8], a) : a;
  }
  for (int w = 1; w < 8; w *= 2)
    for (int k = 0; k < 8; k += 2 * w) b[k] = b[k] + b[k + w];
  return b[0];
}
__global__ void __launch_bounds__(64) k_hildreth_any(int64_t n, int Nc, int nC, const double *Ei, const double *Fi,
                                                     const double *Mi, const double *gi, double *lami, int maxIter,
                                                     double tol, double *DUo, int *nexec, double *scr) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double *E = Ei + (size_t)c * Nc * Nc, *F = Fi + (size_t)c * Nc, *M = Mi + (size_t)c * nC * Nc,
               *gam = gi + (size_t)c * nC;
  double *lam = lami + (size_t)c * nC;
  double *X = scr + (size_t)c * (nC * Nc + 2 * nC), *Hd = X + nC * Nc, *K = Hd + nC;
  double R[HANY_NC * HANY_NC], y[HANY_NC], v[HANY_NC];
  const bool ok = chol_rt(Nc, E, R);
  for (int i = 0; i < nC; ++i) mldiv_rt(Nc, E, R, ok, M + i * Nc, X + i * Nc);  // X(:,i) = E\M(i,:)'
  mldiv_rt(Nc, E, R, ok, F, y);
  bool fin = true;
  for (int i = 0; i < nC; ++i) {
    double s = 0.0, h = 0.0;
    for (int k = 0; k < Nc; ++k) {
      s = s + M[i * Nc + k] * y[k];
      h = h + M[i * Nc + k] * X[i * Nc + k];
      fin = fin && isfinite(X[i * Nc + k]) && isfinite(M[i * Nc + k]);
    }
    K[i] = s + gam[i];
    Hd[i] = h;
  }
  auto xv = [&]() {
    for (int k = 0; k < Nc; ++k) {
      double a = 0.0;
      for (int j = 0; j < nC; ++j) a = __builtin_fma(X[j * Nc + k], lam[j], a);
      v[k] = a;
    }
  };
  int it;
  for (it = 1; it <= maxIter; ++it) {
    bool conv = true;
    if (fin) xv();
    for (int i = 0; i < nC; ++i) {
      const double hii = Hd[i];
      double nl, d;
      if (fin) {
        const double t = row_t_rt(Nc, M + i * Nc, v, K[i]);
        d = hild_step(t, hii, 1.0 / hii, lam[i], nl);
      } else {
        double p4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < nC; ++j) {
          double h = 0.0;
          for (int k = 0; k < Nc; ++k) h = h + M[i * Nc + k] * X[j * Nc + k];
          p4[j & 3] = p4[j & 3] + h * lam[j];
        }
        const double s = (p4[0] + p4[1]) + (p4[2] + p4[3]);
        const double w = -((K[i] + s) - hii * lam[i]) / hii;
        nl = w > 0 ? w : 0.0;
        d = nl - lam[i];
      }
      if (!(fabs(d) < tol)) conv = false;
      lam[i] = nl;
      if (fin) {
        if (isfinite(d)) {
          for (int k = 0; k < Nc; ++k) v[k] = __builtin_fma(X[i * Nc + k], d, v[k]);
        } else {
          xv();
        }
      }
    }
    if (conv) break;
  }
  if (it > maxIter) it = maxIter;
  double rhs[HANY_NC], mE[HANY_NC * HANY_NC], DU[HANY_NC];
  for (int k = 0; k < Nc; ++k) {
    double s = 0.0;
    for (int i = 0; i < nC; ++i) s = s + M[i * Nc + k] * lam[i];
    rhs[k] = F[k] + s;
  }
  for (int i = 0; i < Nc * Nc; ++i) mE[i] = -E[i];
  lu_rt(Nc, mE, rhs, DU);
  for (int k = 0; k < Nc; ++k) DUo[(size_t)c * Nc + k] = DU[k];
  nexec[c] = it;
}

// The fused solver (hild_fast + hild_slow, as k_hild + k_hild_slow) on constraintsMPC.m-structured
// problems given by their Toeplitz rows: M = [Cu; -Cu; I; -I; G_v; -G_e; G_soc].
template <bool SLOW>
__global__ void __launch_bounds__(256) k_hildreth_structured(int64_t n, const double *Ei, const double *Fi,
                                                             const double *Hvi, const double *Hei,
                                                             const double *Hsi, const double *gi, double *lami,
                                                             int maxIter, double tol, double *DUo, int *nexec) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool real = c < n;  // lanes past n ride along (hild_fast keeps the wave full)
  const int64_t cc = real ? c : 0;
  Cons Cn;
  double E[NC][NC], F[NC], K[NCON], lam[NCON];
  if (!real) {
    hild_dummy(Cn, E, K);
#pragma unroll
    for (int i = 0; i < NCON; ++i) lam[i] = 0.0;
#pragma unroll
    for (int a = 0; a < NC; ++a) F[a] = 0.0;
  } else {
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      F[a] = Fi[cc * NC + a];
#pragma unroll
      for (int b = 0; b < NC; ++b) E[a][b] = Ei[(cc * NC + a) * NC + b];
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      Cn.Hv[i] = Hvi[cc * NP + i];
      Cn.He[i] = Hei[cc * NP + i];
      Cn.Hs[i] = Hsi[cc * NP + i];
    }
    double y[NC], R[NC][NC];
    bool ok = chol_n<NC>(E, R);
    mldiv_spd<NC>(E, R, ok, F, y);
    ConsM Mf{Cn};
#pragma unroll
    for (int i = 0; i < NCON; ++i) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) sum = sum + Mf(i, k) * y[k];
      K[i] = sum + gi[cc * NCON + i];
      lam[i] = lami[cc * NCON + i];
    }
  }
  extern __shared__ double2 hlds[];
  int it;
  bool slow = false;
  if (SLOW) {
    slow = real && nexec[cc] < 0;
    if (!__any(slow)) return;
    if (!slow) {  // a finished problem rides along as a passenger
      hild_dummy(Cn, E, K);
#pragma unroll
      for (int i = 0; i < NCON; ++i) lam[i] = 0.0;
    }
    it = hild_slow(Cn, E, lam, maxIter, tol, K, !slow, hild_lane_lds(hlds));
    if (!slow) return;
  } else {
    if (hild_fast(Cn, E, lam, maxIter, tol, K, !real, hild_lane_lds(hlds), lami + cc * NCON, 1, it)) {
      if (real) nexec[cc] = -1;  // the second launch finishes it (warm start still in lambda)
      return;
    }
  }
  double Mtl[NC];
  hild_mtl(Cn, lam, Mtl);
  if (!real) return;
  double rhs[NC], mE[NC][NC], DU[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    rhs[a] = F[a] + Mtl[a];
#pragma unroll
    for (int b = 0; b < NC; ++b) mE[a][b] = -E[a][b];
  }
  lu_solve_n<NC>(mE, rhs, DU);
#pragma unroll
  for (int i = 0; i < NCON; ++i) lami[cc * NCON + i] = lam[i];
#pragma unroll
  for (int a = 0; a < NC; ++a) DUo[cc * NC + a] = DU[a];
  nexec[cc] = it;
}

// initKF.m:94-95 / OB_step.m:185: xhat = 0, SigmaX = SigmaX0(1:5,1:5), bigX = 0
__global__ void k_init_state(int64_t n, int NM, double *ekf, double *bigx, double s0, double s1, double s2, double s3,
                             double s4) {
  const double d[NX] = {s0, s1, s2, s3, s4};
  int64_t total = n * NM;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    double *rec = ekf + i * REC;
#pragma unroll
    for (int k = 0; k < NX; ++k) rec[k] = 0.0;
#pragma unroll
    for (int p = 0; p < NX; ++p)
#pragma unroll
      for (int q = p; q < NX; ++q) rec[NX + pk(p, q)] = p == q ? d[p] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) bigx[i * 6 + k] = 0.0;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_init_state(int64_t n, int NM, double *ekf, double *bigx, const double *sx0, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_init_state, dim3(2048), dim3(256), 0, (hipStream_t)stream, n, NM, ekf, bigx, sx0[0], sx0[1],
                     sx0[2], sx0[3], sx0[4]);
  return (int)hipGetLastError();
}
static int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }

// Compute units of the current device (cached per device).
static int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!cached[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cached[dev] = v;
  }
  return cached[dev];
}
// Block size of a kernel whose blocks each take a CU's LDS (k_cell's ROM blob, k_hild's slots,
// k_bounds' model blob), lpc lanes per cell, launch bound maxb: the fewest 64-lane waves per
// block that still cover the batch in one round of blocks over the CUs.  A small batch then
// runs one wave per CU (configs[1]: 16 CUs) instead of four waves on each of n/256 CUs sharing
// the CU's LDS, L1 and address units; from 64 x #CUs x 4 lanes up it is maxb as before.
// MPCEKF_SPREAD=0: always maxb (A/B; results identical, every lane's arithmetic is its own).
int spread_block(int64_t n, int lpc, int maxb) {
  const char *e = std::getenv("MPCEKF_SPREAD");  // read per launch: tests toggle it in-process
  if (e && std::atoi(e) == 0) return maxb;
  const int64_t lanes = n * lpc, cus = cu_count();
  int64_t b = (lanes + cus - 1) / cus;
  b = (b + 63) / 64 * 64;
  return (int)(b < 64 ? 64 : b > maxb ? maxb : b);
}

int cell_lds_bytes(const KRom &r) {
  return (int)((r.cell_len - (r.rom_global ? r.cell_tab : 0) + 1) * sizeof(double));
}
int bounds_lds_bytes(const KRom &r, int block) { return (bounds_c0_base(r) + block / 4 * 8) * (int)sizeof(double); }
int plant_lds_bytes(const KRom &r) {
  return (int)((r.plant_len - (r.rom_global ? r.plant_tab : 0) + 1) * sizeof(double));
}

bool cell_kernel_supported(int nzp) { return nzp == 26 || nzp == 32; }

// The <GR, PL> of a launch, handed to f as two std::bool_constant values.  GR: the model rows
// are read from the global blob (only the tables staged in LDS); PL: the ABI v3 polynomial
// tables.
template <class F>
static void with_gr_pl(bool global, bool poly, F &&f) {
  using Y = std::true_type;
  using N = std::false_type;
  if (poly) {
    if (global) f(Y{}, Y{});
    else f(N{}, Y{});
  } else {
    if (global) f(Y{}, N{});
    else f(N{}, N{});
  }
}

int launch_plant(const KRom &r, const KState &s, const double *iapp, double *vout, int lazy_t, const double *tc_in,
                 void *stream) {
  if (s.n == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int lds = plant_lds_bytes(r);
  const int block = spread_block(s.n, 4, PLANT4_BLOCK);
  const dim3 g(grid_for(4 * s.n, block)), b(block);
  with_gr_pl(r.rom_global, r.npoly, [&](auto gr, auto pl) {
    hipLaunchKernelGGL((k_plant4<decltype(gr)::value, decltype(pl)::value>), g, b, lds, st, r, s, iapp, vout, lazy_t,
                       tc_in);
  });
  return (int)hipGetLastError();
}

int obs_lds_bytes(const KObs &o) { return (int)((o.len - (o.global ? o.tab : 0) + 1) * sizeof(double)); }

// dynamic LDS above the 64 KiB default (the obs blob: all nz rows of every model, from ~40 models)
static void max_lds_attr(const void *kern) {
  (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

int launch_plant_obs(const KRom &r, const KState &s, const KObs &o, const double *iapp, void *stream) {
  if (s.n == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int lds = obs_lds_bytes(o);
  const int block = spread_block(s.n, 4, OBS_BLOCK);
  const dim3 g(grid_for(4 * s.n, block)), b(block);
  with_gr_pl(o.global, r.npoly, [&](auto gr, auto pl) {
    const auto kern = k_plant_obs<decltype(gr)::value, decltype(pl)::value>;
    max_lds_attr((const void *)kern);
    hipLaunchKernelGGL(kern, g, b, lds, st, r, s, o, iapp);
  });
  return (int)hipGetLastError();
}

int launch_obs_traj(const KRom &r, const KState &s, const KObs &o, const KObsSel &q, int lazy_t, const double *tc_in,
                    void *stream) {
  if (s.n == 0 || q.nsel == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int lds = obs_lds_bytes(o);
  const int block = spread_block(s.n, 4, OBS_BLOCK);
  const dim3 g(grid_for(4 * s.n, block)), b(block);
  with_gr_pl(o.global, r.npoly, [&](auto gr, auto pl) {
    const auto kern = k_obs_traj<decltype(gr)::value, decltype(pl)::value>;
    max_lds_attr((const void *)kern);
    hipLaunchKernelGGL(kern, g, b, lds, st, r, s, o, q, lazy_t, tc_in);
  });
  return (int)hipGetLastError();
}

int launch_flush(const KRom &r, const KCfg &c, const KState &s, int t, int new_ts, void *stream, int64_t c_lo,
                 int64_t c_hi) {
  if (c_hi < 0 || c_hi > s.n) c_hi = s.n;
  if (c_lo < 0) c_lo = 0;
  if (c_hi <= c_lo) return 0;
  static_assert((LAZY_H & (LAZY_H - 1)) == 0 && LAZY_H <= 64, "k_flush: ring slots live in lanes");
  // persistent waves striding over cells, as many as fit: 2 per SIMD with the pipelined
  // loads (210 VGPRs)
  const int64_t wmax = 2048;
  const int64_t waves = c_hi - c_lo < wmax ? c_hi - c_lo : wmax;
  hipLaunchKernelGGL(k_flush, dim3((int)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, r, c, s, t, new_ts,
                     c_lo, c_hi);
  return (int)hipGetLastError();
}

int launch_bulk(const KRom &r, const KCfg &c, const KState &s, const double *iapp, int do_plant, int do_ekf,
                void *stream) {
  if (s.n == 0) return 0;
  int lds = (int)((r.NM * REC + r.NM * 6) * sizeof(double));
  int grid = (int)(s.n < 2048 ? s.n : 2048);
  hipLaunchKernelGGL(k_bulk, dim3(grid), dim3(256), lds, (hipStream_t)stream, r, c, s, iapp, do_plant, do_ekf);
  return (int)hipGetLastError();
}

template <int NZ, int PARTS, bool MB>
static void launch_cell_t(const KRom &r, const KCfg &c, const KState &s, const KIO &io, hipStream_t st) {
  const int block = spread_block(s.n, 1, 256);
  const int lds = cell_lds_bytes(r);
  with_gr_pl(r.rom_global, r.npoly, [&](auto gr, auto pl) {
    const auto kern = k_cell<NZ, PARTS, MB, decltype(gr)::value, decltype(pl)::value>;
    static bool attr = false;  // one per instantiation
    if (!attr) {
      max_lds_attr((const void *)kern);
      attr = true;
    }
    hipLaunchKernelGGL(kern, dim3(grid_for(s.n, block)), dim3(block), lds, st, r, c, s, io);
  });
}

template <int NZ>
static int launch_cell_nz(const KRom &r, const KCfg &c, const KState &s, const KIO &io, hipStream_t st, int parts) {
  if (c.flags & KF_MB) {  // the model-blend EKF ('MB'): fused 5/2, wide (EKF + linearisation) and all stages
    switch (parts) {
      case P_ALL: launch_cell_t<NZ, P_ALL, true>(r, c, s, io, st); return 0;
      case P_EKF | P_LIN: launch_cell_t<NZ, P_EKF | P_LIN, true>(r, c, s, io, st); return 0;
      default: return -1;
    }
  }
  switch (parts) {
    case P_EKF: launch_cell_t<NZ, P_EKF, false>(r, c, s, io, st); return 0;
    case P_MPC: launch_cell_t<NZ, P_MPC, false>(r, c, s, io, st); return 0;
    case P_ALL: launch_cell_t<NZ, P_ALL, false>(r, c, s, io, st); return 0;
    case P_EKF | P_LIN: launch_cell_t<NZ, P_EKF | P_LIN, false>(r, c, s, io, st); return 0;
    default: return -1;
  }
}

int launch_cell(const KRom &r, const KCfg &c, const KState &s, const KIO &io, void *stream, int parts) {
  if (s.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc = -1;
  switch (r.nzp) {
    case 26: rc = launch_cell_nz<26>(r, c, s, io, st, parts); break;
    case 32: rc = launch_cell_nz<32>(r, c, s, io, st, parts); break;
    default: return -1;
  }
  if (rc) return rc;
  return (int)hipGetLastError();
}

template <int NZ, int BLOCK>
static void launch_ekf4_t(const KRom &r, const KCfg &c, const KState &s, const KIO &io, hipStream_t st) {
  // BLOCK is the launch bound; the 256 instantiation (512 registers, no spills) runs the
  // fewest waves per block that cover the batch in one round of CUs (spread_block)
  const int block = BLOCK == 256 ? spread_block(s.n, 4, 256) : BLOCK;
  with_gr_pl(r.rom_global, r.npoly, [&](auto gr, auto pl) {
    const auto kern = k_ekf4<NZ, BLOCK, decltype(gr)::value, decltype(pl)::value>;
    static bool attr = false;  // one per instantiation
    if (!attr) {
      max_lds_attr((const void *)kern);
      attr = true;
    }
    hipLaunchKernelGGL(kern, dim3(grid_for(s.n * 4, block)), dim3(block), cell_lds_bytes(r), st, r, c, s, io);
  });
}

// block = 256 (the small-batch mapping: 512 registers, one wave per SIMD, spread over the
// CUs), 512 (128 cells, 256 VGPRs, 2 waves per SIMD) or 1024 (256 cells, 128 VGPRs, 4 waves
// per SIMD)
int launch_ekf4(const KRom &r, const KCfg &c, const KState &s, const KIO &io, void *stream, int block) {
  if (s.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (r.nzp) {
    case 26:
      if (block == 1024) launch_ekf4_t<26, 1024>(r, c, s, io, st);
      else if (block == 512) launch_ekf4_t<26, 512>(r, c, s, io, st);
      else launch_ekf4_t<26, 256>(r, c, s, io, st);
      break;
    case 32:
      if (block == 1024) launch_ekf4_t<32, 1024>(r, c, s, io, st);
      else if (block == 512) launch_ekf4_t<32, 512>(r, c, s, io, st);
      else launch_ekf4_t<32, 256>(r, c, s, io, st);
      break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

template <int NZ, bool GR>
static void launch_bounds_g(const KRom &r, const KState &s, const double *bnd, double *zbk, hipStream_t st) {
  static bool attr = false;
  const int block = spread_block(s.n, 4, BOUNDS_BLOCK);
  int lds = bounds_lds_bytes(r, block);
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)k_bounds<NZ, GR>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((k_bounds<NZ, GR>), dim3(grid_for(4 * s.n, block)), dim3(block), lds, st, r, s, bnd, zbk);
}

template <int NZ>
static void launch_bounds_t(const KRom &r, const KState &s, const double *bnd, double *zbk, hipStream_t st) {
  // k_bounds reads no electrode table: PL fixed
  with_gr_pl(r.rom_global, false,
             [&](auto gr, auto) { launch_bounds_g<NZ, decltype(gr)::value>(r, s, bnd, zbk, st); });
}

int launch_bounds(const KRom &r, const KState &s, const double *bnd, double *zbk, void *stream) {
  if (s.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (r.nzp) {
    case 26: launch_bounds_t<26>(r, s, bnd, zbk, st); break;
    case 32: launch_bounds_t<32>(r, s, bnd, zbk, st); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

static int hild_lds_bytes(int block = 256) {  // 4 waves per 256-thread block; one block per CU (147 KiB of 160)
  static_assert(4 * HILD_LDS_PER_WAVE <= 160 * 1024, "Hildreth slots exceed the LDS");
  return block / 64 * HILD_LDS_PER_WAVE;
}

size_t hildreth_any_scratch(int64_t n, int Nc, int ncon) { return (size_t)n * (size_t)(ncon * Nc + 2 * ncon); }

int launch_cl_diag(const KCfg &c, int64_t n, const double *lin, const double *uk1, double *poles, double *sv,
                   void *stream, const double *lim) {
  if (n == 0) return 0;
  // per-cell limits: k_cl_diag_pc lives in mpcekf_switch.hip, so that this file's code object is
  // the one a scalar context has always run
  if (lim) return launch_cl_diag_pc(c, n, lin, uk1, poles, sv, stream, lim);
  hipLaunchKernelGGL((k_cl_diag<NP, NC>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, c, n, lin,
                     uk1, poles, sv);
  return (int)hipGetLastError();
}

int launch_hild(const KCfg &c, const KState &s, const KIO &io, void *stream) {
  if (s.n == 0) return 0;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)k_hild, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const int block = spread_block(s.n, 1, 256);
  hipLaunchKernelGGL(k_hild, dim3(grid_for(s.n, block)), dim3(block), hild_lds_bytes(block), (hipStream_t)stream, c, s,
                     io);
  const int gs = grid_for(s.n, 64) < 256 ? grid_for(s.n, 64) : 256;
  hipLaunchKernelGGL(k_hild_slow, dim3(gs), dim3(64), HILD_LDS_PER_WAVE, (hipStream_t)stream, c, s, io);
  return (int)hipGetLastError();
}

int launch_predmat(int64_t n, int Np, int Nc, const double *a, const double *C, const double *D, double *Phi,
                   double *G, void *stream) {
  if (Np != NP || Nc != NC) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_predmat, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, n, a, C, D, Phi, G);
  return (int)hipGetLastError();
}

int launch_constraints(const KCfg &c, int64_t n, const double *lin, const double *uk_1, const double *soc_k1,
                       double *M, double *gam, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_constraints, dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, c, n, lin, uk_1,
                     soc_k1, M, gam);
  return (int)hipGetLastError();
}

int launch_hildreth(int64_t n, int Nc, int ncon, const double *E, const double *F, const double *M,
                    const double *gam, double *lam, int max_iter, double tol, double *DU, int *nexec,
                    void *stream, double *scratch) {
  if (n == 0) return 0;
  if (Nc != NC || ncon != NCON) {  // any other size: the runtime-sized form (scratch: hildreth_any_scratch)
    if (Nc < 1 || Nc > HANY_NC || ncon < 1 || ncon > HANY_NCON || !scratch) return -1;
    hipLaunchKernelGGL(k_hildreth_any, dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, n, Nc, ncon, E, F, M,
                       gam, lam, max_iter, tol, DU, nexec, scratch);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(k_hildreth, dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, n, E, F, M, gam, lam,
                     max_iter, tol, DU, nexec);
  return (int)hipGetLastError();
}

int launch_hildreth_structured(int64_t n, const double *E, const double *F, const double *Hv, const double *He,
                               const double *Hs, const double *gam, double *lam, int max_iter, double tol,
                               double *DU, int *nexec, void *stream) {
  if (n == 0) return 0;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)k_hildreth_structured<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_hildreth_structured<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(k_hildreth_structured<false>, dim3(grid_for(n, 256)), dim3(256), hild_lds_bytes(),
                     (hipStream_t)stream, n, E, F, Hv, He, Hs, gam, lam, max_iter, tol, DU, nexec);
  hipLaunchKernelGGL(k_hildreth_structured<true>, dim3(grid_for(n, 256)), dim3(256), hild_lds_bytes(),
                     (hipStream_t)stream, n, E, F, Hv, He, Hs, gam, lam, max_iter, tol, DU, nexec);
  return (int)hipGetLastError();
}

}  // namespace mk
