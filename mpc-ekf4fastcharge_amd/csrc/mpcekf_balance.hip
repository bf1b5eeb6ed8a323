// mpcekf_balance.hip -- passive balancing of pack strings along the fused loop (include/mpcekf.h,
// mpcekf_balance_begin): on a pack context with a balancer, k_pack_bal runs in k_pack's place.
// After fused step t has stored every cell's command in s.uk (and k_term has rested the latched
// ones), it finds each string's smallest soc among its valid cells, switches every cell's bleeder
// by the distance to it (on at dz_on, off at dz_off, held in between), picks the string's limiter
// on the effective commands e = u - b (compensate) or e = u, and stores the applied current, the
// limiter's e plus the cell's own bleed current, into s.uk, s.uk_1 and the step's u row.  Not a
// reference function.
//
// One launch per step, the one k_pack would have been: balancing adds none.  Per cell the kernel
// loads s.uk, the soc row, three parameters, the flag and the record rows it changes, and stores
// s.uk, s.uk_1, the rows asked for, the flag when it changes and the record rows.  Parameters,
// flags and records are slot-major [k][n], so a wave's loads and stores are contiguous.  Plain
// stores, no atomics: every address is written by exactly one lane.
//
// Two reductions per string before any store: an arg-min over (z, lowest index) among the valid
// cells, and, once every lane knows zmin and with it its own b and e, the arg-max over
// (e, lowest index) among the cells with a command.  Both are exact and associative, so the
// order of the tree does not reach the bits; every combine below still applies the whole rule
// (value first, then the lower index), so it holds across lanes, waves and loop trips.  The
// mapping follows the string length S, as k_pack's does:
//   S == 1            k_pack_bal_one, a lane per cell: the cell is its own string.
//   2 <= S <= 256     k_pack_bal_small: a block of 256 lanes holds floor(256 / S) whole strings, a
//                     lane per cell.  Each reduction is a segmented __shfl_down tree inside a
//                     wave, one LDS hand-off by the head lane of every part of a string (the
//                     string's first lane, or lane 0 of a wave the string continues into) and,
//                     after one barrier, a combine of the string's one to five parts in index
//                     order.  The two reductions use two pairs of hand-off arrays, so the second
//                     needs no barrier to protect the first.
//   S > 256           k_pack_bal_long: a block per string.  Three strided walks: the arg-min, the
//                     arg-max (each cell's e recomputed from zmin), the stores (recomputed once
//                     more: nothing per cell is kept between walks, so S is unbounded).  A lane
//                     visits the same cells in every walk, and only the last walk stores; the
//                     barriers stand where k_pack_long's does, after each reduction's loads.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_balance.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

constexpr int WAVE = 64;
static_assert(PACK_BLOCK % WAVE == 0, "whole waves");

// (bv, bi) <- the better of (bv, bi) and (ov, oi); an index < 0: no cell yet.  By value, so
// -0.0 == +0.0; equal values keep the lower index.  MIN: the smaller value wins, else the larger.
template <bool MIN>
__device__ __forceinline__ void bal_take(double &bv, int &bi, double ov, int oi) {
  if (oi >= 0 && (bi < 0 || (MIN ? ov < bv : ov > bv) || (ov == bv && oi < bi))) {
    bv = ov;
    bi = oi;
  }
}

// one cell's step 2 and 3 of the rule once its string's zmin is known
struct BalCell {
  double d, b, e;
  int on0, on1;  // the flag before and after this step
  bool valid, bleeding;
};

__device__ __forceinline__ BalCell bal_eval(const KPackBal &q, int64_t c, double u, double z, double zmin) {
  const int64_t n = q.p.n;
  BalCell r;
  r.valid = u == u && z == z;
  r.on0 = q.on[c];
  r.on1 = 0;
  r.d = __builtin_nan("");
  if (r.valid) {
    r.d = z - zmin;
    r.on1 = r.d >= q.par[BLP_DZ_ON * n + c] ? 1 : r.d <= q.par[BLP_DZ_OFF * n + c] ? 0 : r.on0;
  }
  const double ib = q.par[BLP_I_BLEED * n + c];
  r.bleeding = r.on1 && ib > 0.0;
  r.b = r.bleeding ? ib : 0.0;
  r.e = q.compensate && r.bleeding && u < 0.0 ? u - r.b : u;
  return r;
}

// one cell's stores once its string's current m and limiter lim are known
__device__ __forceinline__ void bal_cell(const KPackBal &q, int64_t c, int idx, double u, const BalCell &r, double m,
                                         int lim) {
  const int64_t n = q.p.n;
  if (q.p.ucmd) q.p.ucmd[c] = u;
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

__global__ void __launch_bounds__(PACK_BLOCK) k_bal_reset(double *rec, int *on, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
  rec[BL_STEPS_ON * n + c] = 0.0;
  rec[BL_Q_BLEED * n + c] = 0.0;
  rec[BL_SWITCHES * n + c] = 0.0;
  rec[BL_DZ_MAX * n + c] = NaN;
  rec[BL_DZ_LAST * n + c] = NaN;
  rec[BL_STEPS * n + c] = 0.0;
  on[c] = 0;
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_bal_one(KPackBal q) {
  const int64_t c = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (c >= q.p.n) return;
  const double u = q.p.uk[c], z = q.soc[c];
  const double zmin = u == u ? z : __builtin_nan("");  // z itself, or NaN when z is
  const BalCell r = bal_eval(q, c, u, z, zmin);
  if (q.p.limiter) q.p.limiter[c] = u == u ? 0 : -1;
  if (q.zmin) q.zmin[c] = zmin;
  bal_cell(q, c, 0, u, r, r.e, 0);
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_bal_small(KPackBal q) {
  __shared__ double zv[PACK_BLOCK], ev[PACK_BLOCK];
  __shared__ int zi[PACK_BLOCK], ei[PACK_BLOCK];
  const int S = q.p.series, tid = (int)threadIdx.x, lane = tid & (WAVE - 1);
  const int spb = PACK_BLOCK / S;  // strings per block, >= 1
  const int ls = tid / S, idx = tid - ls * S;
  const int64_t nstr = q.p.n / S, g = (int64_t)blockIdx.x * spb + ls;
  const bool live = ls < spb && g < nstr;
  const int64_t c = g * S + idx;  // < n for a live lane
  const int t0 = tid - idx;       // the string's first lane
  const double u = live ? q.p.uk[c] : __builtin_nan("");
  const double z = live ? q.soc[c] : __builtin_nan("");
  // the arg-min of z over the valid cells.  Lane L ends round `off` with the result over
  // [L, L + 2 off) cut at the string's and the wave's end: the partner L + off lies in the same
  // string exactly when idx + off < S (an idle lane has no cell, index -1, and a live lane
  // never pairs with one)
  double bv = z;
  int bi = u == u && z == z ? idx : -1;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (lane + off < WAVE && idx + off < S) bal_take<true>(bv, bi, ov, oi);
  }
  if (idx == 0 || lane == 0) {
    zv[tid] = bv;
    zi[tid] = bi;
  }
  __syncthreads();
  double zmin = __builtin_nan("");
  BalCell r{};
  bv = u;
  bi = -1;
  if (live) {
    double v = zv[t0];
    int k = zi[t0];
    for (int p = (t0 / WAVE + 1) * WAVE; p < t0 + S; p += WAVE) bal_take<true>(v, k, zv[p], zi[p]);
    if (k >= 0) zmin = v;
    r = bal_eval(q, c, u, z, zmin);
    bv = r.e;
    bi = u == u ? idx : -1;
  }
  // the arg-max of e over the cells with a command, the same tree
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (lane + off < WAVE && idx + off < S) bal_take<false>(bv, bi, ov, oi);
  }
  if (idx == 0 || lane == 0) {
    ev[tid] = bv;
    ei[tid] = bi;
  }
  __syncthreads();
  if (!live) return;
  double m = ev[t0];
  int lim = ei[t0];
  for (int p = (t0 / WAVE + 1) * WAVE; p < t0 + S; p += WAVE) bal_take<false>(m, lim, ev[p], ei[p]);
  if (idx == 0) {
    if (q.p.limiter) q.p.limiter[g] = lim;
    if (q.zmin) q.zmin[g] = zmin;
  }
  bal_cell(q, c, idx, u, r, m, lim);
}

// the wave's result into lane 0, then the block's from LDS into every lane
template <bool MIN>
__device__ __forceinline__ void bal_block(double &bv, int &bi, double *pv, int *pi, int tid) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    bal_take<MIN>(bv, bi, ov, oi);  // lanes past WAVE - off read their own value back: no change
  }
  if ((tid & (WAVE - 1)) == 0) {
    pv[tid / WAVE] = bv;
    pi[tid / WAVE] = bi;
  }
  __syncthreads();  // also: every load of the walk before is done before the stores of the last walk
  bv = pv[0];
  bi = pi[0];
#pragma unroll
  for (int w = 1; w < PACK_BLOCK / WAVE; ++w) bal_take<MIN>(bv, bi, pv[w], pi[w]);
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_bal_long(KPackBal q) {
  __shared__ double zv[PACK_BLOCK / WAVE], ev[PACK_BLOCK / WAVE];
  __shared__ int zi[PACK_BLOCK / WAVE], ei[PACK_BLOCK / WAVE];
  const int S = q.p.series, tid = (int)threadIdx.x;
  const int64_t g = blockIdx.x, base = g * S;  // the grid is n / S blocks
  double bv = __builtin_nan("");
  int bi = -1;
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = q.p.uk[base + i], z = q.soc[base + i];
    if (u == u && z == z) bal_take<true>(bv, bi, z, i);
  }
  bal_block<true>(bv, bi, zv, zi, tid);
  const double zmin = bi >= 0 ? bv : __builtin_nan("");
  bv = __builtin_nan("");
  bi = -1;
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = q.p.uk[base + i];
    if (u == u) bal_take<false>(bv, bi, bal_eval(q, base + i, u, q.soc[base + i], zmin).e, i);
  }
  bal_block<false>(bv, bi, ev, ei, tid);
  const double m = bv;
  const int lim = bi;
  if (tid == 0) {
    if (q.p.limiter) q.p.limiter[g] = lim;
    if (q.zmin) q.zmin[g] = zmin;
  }
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = q.p.uk[base + i];
    bal_cell(q, base + i, i, u, bal_eval(q, base + i, u, q.soc[base + i], zmin), m, lim);
  }
}

unsigned bal_grid(int64_t n) { return (unsigned)((n + PACK_BLOCK - 1) / PACK_BLOCK); }

}  // namespace

int launch_bal_reset(double *rec, int *on, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_bal_reset, dim3(bal_grid(n)), dim3(PACK_BLOCK), 0, (hipStream_t)stream, rec, on, n);
  return (int)hipGetLastError();
}

int launch_pack_bal(const KPackBal &q, void *stream) {
  const int64_t n = q.p.n;
  const int S = q.p.series;
  if (n <= 0 || S < 1 || n % S) return 0;
  const int64_t nstr = n / S;
  if (S == 1) {
    hipLaunchKernelGGL(k_pack_bal_one, dim3(bal_grid(n)), dim3(PACK_BLOCK), 0, (hipStream_t)stream, q);
  } else if (S <= PACK_BLOCK) {
    const int64_t spb = PACK_BLOCK / S;
    hipLaunchKernelGGL(k_pack_bal_small, dim3((unsigned)((nstr + spb - 1) / spb)), dim3(PACK_BLOCK), 0,
                       (hipStream_t)stream, q);
  } else {
    hipLaunchKernelGGL(k_pack_bal_long, dim3((unsigned)nstr), dim3(PACK_BLOCK), 0, (hipStream_t)stream, q);
  }
  return (int)hipGetLastError();
}

}  // namespace mk
