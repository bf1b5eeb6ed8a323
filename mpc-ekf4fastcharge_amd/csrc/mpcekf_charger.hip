// mpcekf_charger.hip -- charger limits on pack strings along the fused loop (include/mpcekf.h,
// mpcekf_charger_begin): on a pack context with a charger, k_charger runs in k_pack's or
// k_pack_bal's place.  After fused step t has stored every cell's command in s.uk (and k_term has
// rested the latched ones), it adds up each string's terminal voltage from the cells' s.vk, runs
// the balancer's steps when the context has one, picks the string's limiter and current as the
// pack does, raises that current to the charger's current and power caps (charging current is
// negative: a cap is a lower bound) and stores the applied current into s.uk, s.uk_1 and the
// step's u row.  Not a reference function.
//
// One launch per step, the one k_pack or k_pack_bal would have been: the charger adds none.
// Plain stores, no atomics: every address is written by exactly one lane (a string's rows and
// record by the lane of its first cell).  The helpers of mpcekf_pack.hip / mpcekf_balance.hip are
// restated here, not shared, so those two units stay what they were.
//
// The string voltage is the project's first floating-point sum across cells, and a sum is not
// associative: the header fixes its shape, a binary tree over the in-string index (level j adds
// x[i + 2^j] into x[i] for every i that is a multiple of 2^(j+1)), and every mapping below
// realises that shape whatever block, wave or lane a cell sits in.  The arg-min and arg-max are
// exact and keep the tree shapes of k_pack_bal.  The mapping follows the string length S:
//   S == 1            k_charger_one, a lane per cell: V = v + 0.0.
//   2 <= S <= 256     k_charger_small: a block of 256 lanes holds floor(256 / S) whole strings, a
//                     lane per cell.  A string starts at any lane and may straddle a wave
//                     boundary, so the tree runs in LDS on the in-string index: one barrier per
//                     level, ceil(log2 S) levels.  At a level the lanes that add (index a
//                     multiple of 2^(j+1)) and the entries they read (index an odd multiple of
//                     2^j) are disjoint, so one barrier per level is enough.  The count of the
//                     cells that contributed rides the same tree.
//   S > 256           k_charger_long: a block per string.  The string is cut into tiles of 256
//                     cells aligned on the in-string index; a tile is a whole subtree (levels
//                     0..7): __shfl_down inside a wave gives lane 0 the aligned tree over its 64
//                     cells, the four wave sums meet in LDS as (w0 + w1) + (w2 + w3).  Lane 0 of
//                     the block combines the tile sums in tree order with a stack of pending
//                     partials, one per level, as in pairwise summation: after tile k it merges
//                     once per trailing one bit of k, and after the last tile it folds what is
//                     left from the top, which is the tree with the missing partners skipped.
//                     The stack lives in LDS (32 entries: more levels than an int32 S has), so
//                     LDS is constant in S and nothing is indexed dynamically in registers.  The
//                     wave sums are double-buffered on the tile's parity: one barrier per tile.
// A cell beyond S, or one whose command or voltage is NaN, enters as +0.0.  No term is -0.0 (x =
// v + 0.0), so no partial sum is, and adding +0.0 equals skipping the partner.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_charger.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

constexpr int WAVE = 64;
constexpr int NWAVE = PACK_BLOCK / WAVE;
constexpr int CH_STACK = 32;  // pending partials: one per level above a tile
static_assert(PACK_BLOCK % WAVE == 0, "whole waves");
static_assert(NWAVE == 4, "the tile's wave sums are combined as (w0 + w1) + (w2 + w3)");

// (bv, bi) <- the better of (bv, bi) and (ov, oi); an index < 0: no cell yet.  By value, so
// -0.0 == +0.0; equal values keep the lower index.  MIN: the smaller value wins, else the larger.
template <bool MIN>
__device__ __forceinline__ void ch_take(double &bv, int &bi, double ov, int oi) {
  if (oi >= 0 && (bi < 0 || (MIN ? ov < bv : ov > bv) || (ov == bv && oi < bi))) {
    bv = ov;
    bi = oi;
  }
}

// one cell's step 2 and 3 of the balance rule once its string's zmin is known; without a
// balancer: no bleeder, e = u
struct ChCell {
  double d, b, e;
  int on0, on1;  // the flag before and after this step
  bool valid, bleeding;
};

template <bool BAL>
__device__ __forceinline__ ChCell ch_eval(const KPackBal &q, int64_t c, double u, double z, double zmin) {
  ChCell r;
  r.valid = false;
  r.on0 = r.on1 = 0;
  r.d = __builtin_nan("");
  r.bleeding = false;
  r.b = 0.0;
  r.e = u;
  if (BAL) {
    const int64_t n = q.p.n;
    r.valid = u == u && z == z;
    r.on0 = q.on[c];
    if (r.valid) {
      r.d = z - zmin;
      r.on1 = r.d >= q.par[BLP_DZ_ON * n + c] ? 1 : r.d <= q.par[BLP_DZ_OFF * n + c] ? 0 : r.on0;
    }
    const double ib = q.par[BLP_I_BLEED * n + c];
    r.bleeding = r.on1 && ib > 0.0;
    r.b = r.bleeding ? ib : 0.0;
    r.e = q.compensate && r.bleeding && u < 0.0 ? u - r.b : u;
  }
  return r;
}

// step 4 of the charger's rule: the string current after the caps and which cap set it
struct ChStr {
  double m;  // m'_g; NaN for a string without a current
  int by;    // capby: -1 no current, 0 not capped, 1 the current cap, 2 the power cap
};

__device__ __forceinline__ ChStr ch_caps(const KCharger &q, int64_t g, double V, double m, int lim) {
  ChStr s;
  s.m = __builtin_nan("");
  s.by = -1;
  if (lim < 0) return s;
  const int64_t nstr = q.b.p.n / q.b.p.series;
  const double imax = q.par[CHP_I_MAX * nstr + g], pmax = q.par[CHP_P_MAX * nstr + g];
  double cap = 0.0;
  int by = 0;
  if (imax == imax) {
    cap = -imax;
    by = 1;
  }
  if (pmax == pmax && V > 0.0) {
    const double cp = -(pmax / V);
    if (by == 0 || cp > cap) {  // a tie keeps the current cap
      cap = cp;
      by = 2;
    }
  }
  if (by != 0 && cap > m) {
    s.m = cap;
    s.by = by;
  } else {
    s.m = m;
    s.by = 0;
  }
  return s;
}

// the string's rows and record, by the lane of its first cell; m: the current before the caps
__device__ __forceinline__ void ch_string(const KCharger &q, int64_t g, double V, int nvalid, double m, int lim,
                                          const ChStr &s) {
  const int64_t nstr = q.b.p.n / q.b.p.series;
  if (q.b.p.limiter) q.b.p.limiter[g] = s.by > 0 ? -2 : lim;
  if (q.vstr) q.vstr[g] = V;
  if (q.istr) q.istr[g] = s.m;
  if (q.capby) q.capby[g] = s.by;
  if (lim < 0) return;  // no string current: the record counts nothing
  double *R = q.rec + g;
  R[CH_STEPS * nstr] = R[CH_STEPS * nstr] + 1.0;
  if (s.by == 1) R[CH_NCAP_I * nstr] = R[CH_NCAP_I * nstr] + 1.0;
  if (s.by == 2) R[CH_NCAP_P * nstr] = R[CH_NCAP_P * nstr] + 1.0;
  if (__builtin_isfinite(s.m)) R[CH_Q * nstr] = R[CH_Q * nstr] + s.m;
  const double p = V * s.m;
  if (__builtin_isfinite(p)) R[CH_E * nstr] = R[CH_E * nstr] + p;
  const double dm = s.m - m;
  if (__builtin_isfinite(dm)) R[CH_CURTAIL * nstr] = R[CH_CURTAIL * nstr] + dm;
  const double pm = R[CH_P_MIN * nstr];
  if (p == p && (pm != pm || p < pm)) R[CH_P_MIN * nstr] = p;
  const double vp = R[CH_V_PEAK * nstr];
  if (V == V && (vp != vp || V > vp)) R[CH_V_PEAK * nstr] = V;
  const double nv = (double)nvalid, nm = R[CH_NVALID_MIN * nstr];
  if (nm != nm || nv < nm) R[CH_NVALID_MIN * nstr] = nv;
}

// one cell's stores once its string's current after the caps, m, is known; lim: the limiter, or
// -2 on a capped step (no cell is the limiter then)
template <bool BAL>
__device__ __forceinline__ void ch_cell(const KPackBal &q, int64_t c, int idx, double u, const ChCell &r, double m,
                                        int lim) {
  const int64_t n = q.p.n;
  if (q.p.ucmd) q.p.ucmd[c] = u;
  if (BAL) {
    if (r.on1 != r.on0) q.on[c] = r.on1;
    double *B = q.rec + c;
    B[BL_DZ_LAST * n] = r.d;
    if (r.valid) {
      B[BL_STEPS * n] = B[BL_STEPS * n] + 1.0;
      const double dm = B[BL_DZ_MAX * n];
      if (r.d == r.d && (dm != dm || r.d > dm)) B[BL_DZ_MAX * n] = r.d;
    }
    if (r.on1 && !r.on0) B[BL_SWITCHES * n] = B[BL_SWITCHES * n] + 1.0;
    if (r.bleeding) {
      B[BL_STEPS_ON * n] = B[BL_STEPS_ON * n] + 1.0;
      B[BL_Q_BLEED * n] = B[BL_Q_BLEED * n] + r.b;
    }
    if (q.bleed) q.bleed[c] = u == u ? r.b : __builtin_nan("");
  }
  if (u != u) return;  // excluded: keeps its NaN, s.uk_1 untouched, counts nothing in the pack record
  const double a = r.bleeding ? m + r.b : m;
  q.p.uk[c] = a;
  q.p.uk_1[c] = a;
  if (q.p.u) q.p.u[c] = a;
  double *R = q.p.rec + c;
  R[PK_STEPS * n] = R[PK_STEPS * n] + 1.0;
  if (idx == lim) R[PK_NLIM * n] = R[PK_NLIM * n] + 1.0;
  const double h = m - r.e;
  if (__builtin_isfinite(h)) R[PK_HEADROOM * n] = R[PK_HEADROOM * n] + h;
}

__global__ void __launch_bounds__(PACK_BLOCK) k_charger_reset(double *rec, int64_t nstr) {
  const int64_t g = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (g >= nstr) return;
  const double NaN = __builtin_nan("");
  rec[CH_STEPS * nstr + g] = 0.0;
  rec[CH_NCAP_I * nstr + g] = 0.0;
  rec[CH_NCAP_P * nstr + g] = 0.0;
  rec[CH_Q * nstr + g] = 0.0;
  rec[CH_E * nstr + g] = 0.0;
  rec[CH_CURTAIL * nstr + g] = 0.0;
  rec[CH_P_MIN * nstr + g] = NaN;
  rec[CH_V_PEAK * nstr + g] = NaN;
  rec[CH_NVALID_MIN * nstr + g] = NaN;
}

template <bool BAL>
__global__ void __launch_bounds__(PACK_BLOCK) k_charger_one(KCharger q) {
  const KPackBal &b = q.b;
  const int64_t c = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (c >= b.p.n) return;
  const double u = b.p.uk[c], v = q.vk[c];
  const bool term = u == u && v == v;
  const double V = term ? v + 0.0 : 0.0;
  double z = __builtin_nan(""), zmin = z;
  if (BAL) {
    z = b.soc[c];
    zmin = u == u ? z : __builtin_nan("");  // z itself, or NaN when z is
    if (b.zmin) b.zmin[c] = zmin;
  }
  const ChCell r = ch_eval<BAL>(b, c, u, z, zmin);
  const int lim = u == u ? 0 : -1;
  const ChStr s = ch_caps(q, c, V, r.e, lim);
  ch_string(q, c, V, (int)term, r.e, lim, s);
  ch_cell<BAL>(b, c, 0, u, r, s.m, s.by > 0 ? -2 : lim);
}

template <bool BAL>
__global__ void __launch_bounds__(PACK_BLOCK) k_charger_small(KCharger q) {
  __shared__ double xs[PACK_BLOCK], zv[PACK_BLOCK], ev[PACK_BLOCK];
  __shared__ int xn[PACK_BLOCK], zi[PACK_BLOCK], ei[PACK_BLOCK];
  const KPackBal &b = q.b;
  const int S = b.p.series, tid = (int)threadIdx.x, lane = tid & (WAVE - 1);
  const int spb = PACK_BLOCK / S;  // strings per block, >= 1
  const int ls = tid / S, idx = tid - ls * S;
  const int64_t nstr = b.p.n / S, g = (int64_t)blockIdx.x * spb + ls;
  const bool whole = ls < spb;  // the lane's string lies inside the block
  const bool live = whole && g < nstr;
  const int64_t c = g * S + idx;  // < n for a live lane
  const int t0 = tid - idx;       // the string's first lane
  const double u = live ? b.p.uk[c] : __builtin_nan("");
  const double v = live ? q.vk[c] : __builtin_nan("");
  const double z = BAL && live ? b.soc[c] : __builtin_nan("");
  // the string voltage: the header's tree on the in-string index, in LDS.  `whole` keeps
  // tid + off inside the block: idx + off < S stays inside the string
  const bool term = u == u && v == v;
  xs[tid] = term ? v + 0.0 : 0.0;
  xn[tid] = (int)term;
  for (int off = 1; off < S; off <<= 1) {
    __syncthreads();
    if (whole && (idx & (2 * off - 1)) == 0 && idx + off < S) {
      xs[tid] = xs[tid] + xs[tid + off];
      xn[tid] = xn[tid] + xn[tid + off];
    }
  }
  // the arg-min of z over the valid cells, as in k_pack_bal_small: lane L ends round `off` with
  // the result over [L, L + 2 off) cut at the string's and the wave's end
  double zmin = __builtin_nan("");
  double bv = u;
  int bi = u == u ? idx : -1;
  ChCell r = ch_eval<false>(b, c, u, z, zmin);
  if (BAL) {
    bv = z;
    bi = u == u && z == z ? idx : -1;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const double ov = __shfl_down(bv, off);
      const int oi = __shfl_down(bi, off);
      if (lane + off < WAVE && idx + off < S) ch_take<true>(bv, bi, ov, oi);
    }
    if (idx == 0 || lane == 0) {
      zv[tid] = bv;
      zi[tid] = bi;
    }
    __syncthreads();
    bv = u;
    bi = -1;
    if (live) {
      double w = zv[t0];
      int k = zi[t0];
      for (int p = (t0 / WAVE + 1) * WAVE; p < t0 + S; p += WAVE) ch_take<true>(w, k, zv[p], zi[p]);
      if (k >= 0) zmin = w;
      r = ch_eval<true>(b, c, u, z, zmin);
      bv = r.e;
      bi = u == u ? idx : -1;
    }
  }
  // the arg-max of e over the cells with a command, the same tree
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (lane + off < WAVE && idx + off < S) ch_take<false>(bv, bi, ov, oi);
  }
  if (idx == 0 || lane == 0) {
    ev[tid] = bv;
    ei[tid] = bi;
  }
  __syncthreads();  // also: the last level of the voltage tree is done
  if (!live) return;
  double m = ev[t0];
  int lim = ei[t0];
  for (int p = (t0 / WAVE + 1) * WAVE; p < t0 + S; p += WAVE) ch_take<false>(m, lim, ev[p], ei[p]);
  const double V = xs[t0];
  const ChStr s = ch_caps(q, g, V, m, lim);
  if (idx == 0) {
    if (BAL && b.zmin) b.zmin[g] = zmin;
    ch_string(q, g, V, xn[t0], m, lim, s);
  }
  ch_cell<BAL>(b, c, idx, u, r, s.m, s.by > 0 ? -2 : lim);
}

// the wave's result into lane 0, then the block's from LDS into every lane
template <bool MIN>
__device__ __forceinline__ void ch_block(double &bv, int &bi, double *pv, int *pi, int tid) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    ch_take<MIN>(bv, bi, ov, oi);  // lanes past WAVE - off read their own value back: no change
  }
  if ((tid & (WAVE - 1)) == 0) {
    pv[tid / WAVE] = bv;
    pi[tid / WAVE] = bi;
  }
  __syncthreads();  // also: every load of the walk before is done before the stores of the last walk
  bv = pv[0];
  bi = pi[0];
#pragma unroll
  for (int w = 1; w < NWAVE; ++w) ch_take<MIN>(bv, bi, pv[w], pi[w]);
}

template <bool BAL>
__global__ void __launch_bounds__(PACK_BLOCK) k_charger_long(KCharger q) {
  __shared__ double zv[NWAVE], ev[NWAVE], tw[2][NWAVE], stk[CH_STACK], vres;
  __shared__ int zi[NWAVE], ei[NWAVE], tn[2][NWAVE], nres;
  const KPackBal &b = q.b;
  const int S = b.p.series, tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int64_t g = blockIdx.x, base = g * S;  // the grid is n / S blocks
  // the string voltage, tile by tile; sp and ntot are lane 0's
  int sp = 0, ntot = 0;
  for (int i0 = 0, k = 0; i0 < S; i0 += PACK_BLOCK, ++k) {
    const int i = i0 + tid, h = k & 1;
    double x = 0.0;
    bool term = false;
    if (i < S) {
      const double u = b.p.uk[base + i], v = q.vk[base + i];
      term = u == u && v == v;
      if (term) x = v + 0.0;
    }
    const int cnt = (int)__popcll(__ballot(term));
    // lane 0 ends with the aligned tree over the wave's 64 cells: at round `off` it reads lane
    // `off`, which holds the tree over [off, 2 off); what the other lanes hold is not used
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) x = x + __shfl_down(x, off);
    if (lane == 0) {
      tw[h][wave] = x;
      tn[h][wave] = cnt;
    }
    __syncthreads();  // tile k + 1 writes the other half; tile k + 2 this one, behind tile k + 1's barrier
    if (tid == 0) {
      double T = (tw[h][0] + tw[h][1]) + (tw[h][2] + tw[h][3]);
      ntot += (tn[h][0] + tn[h][1]) + (tn[h][2] + tn[h][3]);
      for (int cbit = k + 1; (cbit & 1) == 0; cbit >>= 1) T = stk[--sp] + T;  // a finished pair, level by level
      stk[sp++] = T;
    }
  }
  if (tid == 0) {  // what is left has no partner at its level: folded from the top
    double V = stk[--sp];
    while (sp > 0) V = stk[--sp] + V;
    vres = V;
    nres = ntot;
  }
  double bv = __builtin_nan("");
  int bi = -1;
  double zmin = __builtin_nan("");
  if (BAL) {
    for (int i = tid; i < S; i += PACK_BLOCK) {
      const double u = b.p.uk[base + i], z = b.soc[base + i];
      if (u == u && z == z) ch_take<true>(bv, bi, z, i);
    }
    ch_block<true>(bv, bi, zv, zi, tid);
    zmin = bi >= 0 ? bv : __builtin_nan("");
    bv = __builtin_nan("");
    bi = -1;
  }
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = b.p.uk[base + i];
    if (u == u) ch_take<false>(bv, bi, ch_eval<BAL>(b, base + i, u, BAL ? b.soc[base + i] : u, zmin).e, i);
  }
  ch_block<false>(bv, bi, ev, ei, tid);  // its barrier also publishes vres and nres
  const double m = bv, V = vres;
  const int lim = bi;
  const ChStr s = ch_caps(q, g, V, m, lim);
  if (tid == 0) {
    if (BAL && b.zmin) b.zmin[g] = zmin;
    ch_string(q, g, V, nres, m, lim, s);
  }
  const int leff = s.by > 0 ? -2 : lim;
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = b.p.uk[base + i];
    ch_cell<BAL>(b, base + i, i, u, ch_eval<BAL>(b, base + i, u, BAL ? b.soc[base + i] : u, zmin), s.m, leff);
  }
}

unsigned ch_grid(int64_t n) { return (unsigned)((n + PACK_BLOCK - 1) / PACK_BLOCK); }

template <bool BAL>
void ch_launch(const KCharger &q, hipStream_t stream) {
  const int64_t n = q.b.p.n;
  const int S = q.b.p.series;
  const int64_t nstr = n / S;
  if (S == 1) {
    hipLaunchKernelGGL(k_charger_one<BAL>, dim3(ch_grid(n)), dim3(PACK_BLOCK), 0, stream, q);
  } else if (S <= PACK_BLOCK) {
    const int64_t spb = PACK_BLOCK / S;
    hipLaunchKernelGGL(k_charger_small<BAL>, dim3((unsigned)((nstr + spb - 1) / spb)), dim3(PACK_BLOCK), 0, stream, q);
  } else {
    hipLaunchKernelGGL(k_charger_long<BAL>, dim3((unsigned)nstr), dim3(PACK_BLOCK), 0, stream, q);
  }
}

}  // namespace

int launch_charger_reset(double *rec, int64_t nstrings, void *stream) {
  if (nstrings <= 0) return 0;
  hipLaunchKernelGGL(k_charger_reset, dim3(ch_grid(nstrings)), dim3(PACK_BLOCK), 0, (hipStream_t)stream, rec, nstrings);
  return (int)hipGetLastError();
}

int launch_charger(const KCharger &q, void *stream) {
  const int64_t n = q.b.p.n;
  const int S = q.b.p.series;
  if (n <= 0 || S < 1 || n % S) return 0;
  if (q.b.par)
    ch_launch<true>(q, (hipStream_t)stream);
  else
    ch_launch<false>(q, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // namespace mk
