// mpcekf_pack.hip -- series strings along the fused loop (include/mpcekf.h, mpcekf_pack_begin):
// the cells [g S, (g + 1) S) of a context form string g, which carries one current.  After
// fused step t has stored every cell's command in s.uk, k_pack picks each string's limiter,
// the cell with the largest command (charging current is negative, initMPC.m:66-67: the
// largest is the smallest charging current) among the cells whose command is not NaN, lowest
// in-string index on a tie, and stores the limiter's command, bit for bit, into s.uk, s.uk_1
// and the step's u row of every such cell of the string.  Not a reference function.
//
// One launch per step, after Hildreth (and k_cl_diag), before the summary fold and k_thermal,
// so the summary's current and charge, the thermal model's carried current and the next step's
// uk_1 all see the applied current.  Per cell the kernel loads s.uk and the three record rows
// (32 B) and stores s.uk, s.uk_1, the three record rows and, when asked for, the u and ucmd
// rows (40-56 B); a cell whose command is NaN stores its ucmd entry only.  Plain stores, no
// atomics: every address is written by exactly one lane.
//
// The reduction is an arg-max over (value, lowest index), which is exact and associative, so
// the order of the tree does not reach the bits; every combine below still applies the whole
// rule (value first, then the lower index), so it holds across lanes, waves and loop trips.
// The mapping follows the string length S:
//   S == 1            k_pack_one, a lane per cell: the cell is its own limiter; only the record
//                     counts, s.uk / s.uk_1 / u keep the bits the step stored.
//   2 <= S <= 256     k_pack_small: a block of 256 lanes holds floor(256 / S) whole strings, a
//                     lane per cell, so no string straddles a block (256 % S lanes idle).  A
//                     segmented __shfl_down tree reduces the part of a string inside one wave;
//                     the head lane of every such part (the string's first lane, or lane 0 of a
//                     wave the string continues into) stores its partial result to LDS, and after
//                     one barrier every lane combines its string's one to five parts in index
//                     order.
//   S > 256           k_pack_long: a block per string.  Each lane walks the string with stride
//                     256, the wave reduces with __shfl_down, the four wave results meet in
//                     LDS, and a second walk (after the barrier: no lane stores s.uk before
//                     every lane has read it) stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_pack.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

constexpr int WAVE = 64;
static_assert(PACK_BLOCK % WAVE == 0, "whole waves");

// (bv, bi) <- the better of (bv, bi) and (ov, oi); an index < 0: no cell yet.  By value, so
// -0.0 == +0.0; equal values keep the lower index.
__device__ __forceinline__ void pack_take(double &bv, int &bi, double ov, int oi) {
  if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
    bv = ov;
    bi = oi;
  }
}

// one cell's stores once its string's current m and limiter lim are known; u: its own command
template <bool COUPLE>
__device__ __forceinline__ void pack_cell(const KPack &q, int64_t c, int idx, double u, double m, int lim) {
  if (q.ucmd) q.ucmd[c] = u;
  if (u != u) return;  // excluded: keeps its NaN, s.uk_1 untouched, counts nothing
  const int64_t n = q.n;
  if (COUPLE) {
    q.uk[c] = m;
    q.uk_1[c] = m;
    if (q.u) q.u[c] = m;
  }
  double *R = q.rec + c;
  R[PK_STEPS * n] = R[PK_STEPS * n] + 1.0;
  if (idx == lim) R[PK_NLIM * n] = R[PK_NLIM * n] + 1.0;
  const double d = m - u;
  if (__builtin_isfinite(d)) R[PK_HEADROOM * n] = R[PK_HEADROOM * n] + d;
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_one(KPack q) {
  const int64_t c = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
  if (c >= q.n) return;
  const double u = q.uk[c];
  if (q.limiter) q.limiter[c] = u == u ? 0 : -1;
  pack_cell<false>(q, c, 0, u, u, 0);
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_small(KPack q) {
  __shared__ double pv[PACK_BLOCK];
  __shared__ int pi[PACK_BLOCK];
  const int S = q.series, tid = (int)threadIdx.x, lane = tid & (WAVE - 1);
  const int spb = PACK_BLOCK / S;  // strings per block, >= 1
  const int ls = tid / S, idx = tid - ls * S;
  const int64_t nstr = q.n / S, g = (int64_t)blockIdx.x * spb + ls;
  const bool live = ls < spb && g < nstr;
  const int64_t c = g * S + idx;  // < n for a live lane
  const double u = live ? q.uk[c] : __builtin_nan("");
  double bv = u;
  int bi = u == u ? idx : -1;
  // lane L ends round `off` with the result over [L, L + 2 off) cut at the string's and the
  // wave's end: the partner L + off lies in the same string exactly when idx + off < S (an
  // idle lane has no cell, index -1, and a live lane never pairs with one)
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (lane + off < WAVE && idx + off < S) pack_take(bv, bi, ov, oi);
  }
  if (idx == 0 || lane == 0) {
    pv[tid] = bv;
    pi[tid] = bi;
  }
  __syncthreads();
  if (!live) return;
  const int t0 = tid - idx;  // the string's first lane
  double m = pv[t0];
  int lim = pi[t0];
  for (int p = (t0 / WAVE + 1) * WAVE; p < t0 + S; p += WAVE) pack_take(m, lim, pv[p], pi[p]);
  if (idx == 0 && q.limiter) q.limiter[g] = lim;
  pack_cell<true>(q, c, idx, u, m, lim);
}

__global__ void __launch_bounds__(PACK_BLOCK) k_pack_long(KPack q) {
  __shared__ double pv[PACK_BLOCK / WAVE];
  __shared__ int pi[PACK_BLOCK / WAVE];
  const int S = q.series, tid = (int)threadIdx.x;
  const int64_t g = blockIdx.x, base = g * S;  // the grid is n / S blocks
  double bv = __builtin_nan("");
  int bi = -1;
  for (int i = tid; i < S; i += PACK_BLOCK) {
    const double u = q.uk[base + i];
    if (u == u) pack_take(bv, bi, u, i);
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    pack_take(bv, bi, ov, oi);  // lanes past WAVE - off read their own value back: no change
  }
  if ((tid & (WAVE - 1)) == 0) {
    pv[tid / WAVE] = bv;
    pi[tid / WAVE] = bi;
  }
  __syncthreads();  // also: every load of s.uk above is done before the stores below
  double m = pv[0];
  int lim = pi[0];
#pragma unroll
  for (int w = 1; w < PACK_BLOCK / WAVE; ++w) pack_take(m, lim, pv[w], pi[w]);
  if (tid == 0 && q.limiter) q.limiter[g] = lim;
  for (int i = tid; i < S; i += PACK_BLOCK) pack_cell<true>(q, base + i, i, q.uk[base + i], m, lim);
}

}  // namespace

int launch_pack(const KPack &q, void *stream) {
  if (q.n <= 0 || q.series < 1 || q.n % q.series) return 0;
  const int64_t nstr = q.n / q.series;
  if (q.series == 1) {
    hipLaunchKernelGGL(k_pack_one, dim3((unsigned)((q.n + PACK_BLOCK - 1) / PACK_BLOCK)), dim3(PACK_BLOCK), 0,
                       (hipStream_t)stream, q);
  } else if (q.series <= PACK_BLOCK) {
    const int64_t spb = PACK_BLOCK / q.series;
    hipLaunchKernelGGL(k_pack_small, dim3((unsigned)((nstr + spb - 1) / spb)), dim3(PACK_BLOCK), 0, (hipStream_t)stream,
                       q);
  } else {
    hipLaunchKernelGGL(k_pack_long, dim3((unsigned)nstr), dim3(PACK_BLOCK), 0, (hipStream_t)stream, q);
  }
  return (int)hipGetLastError();
}

}  // namespace mk
