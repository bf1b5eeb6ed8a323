// mpcekf_term.hip -- charge termination along the fused loop (include/mpcekf.h,
// mpcekf_term_begin): after fused step t has stored every cell's command in s.uk, k_term applies
// the header's rule to each cell: an OPEN cell whose soc row or command is NaN becomes DEAD; one
// whose string held a latched cell after step t - 1 latches with reason 8; otherwise the three
// criteria (SOC reached, current tapered for `hold` steps, temperature cut-off) are evaluated
// and any of them latches the cell.  A latched cell's command becomes +0.0 in s.uk, s.uk_1 and
// the step's u row, so k_pack, the plant, the EKF, the summary, k_aging and k_thermal all see a
// resting cell.  Not a reference function.
//
// One launch per step, after Hildreth (and k_cl_diag), before k_pack.  A lane per cell, blocks
// of 256; every array is slot-major, so a wave's loads and stores are contiguous.  Per OPEN cell
// the kernel loads s.uk, the soc row, s.Tc, three parameters, two counters and two record rows
// (64 B) and stores the counters, STATE and STEPS (24 B); a latched cell loads s.uk, STATE and
// REST and stores s.uk, s.uk_1, the u row and REST.
//
// The string flag: a launch reads flag_in and writes flag_out, two different buffers (the host
// alternates them by the call-relative parity of the step), so the result does not depend on the
// order the blocks run in.  Every latched cell stores 1 into its string's flag_out in every step;
// the lanes of a string all store the same value, and no lane stores 0: flags only rise until
// mpcekf_term_begin.  k_term_seed rebuilds flag_in of a call's first step from the cells' states.
//
// The open counter: each wave counts the cells it closed in this step with a ballot and one
// lane subtracts the count with one atomic add.  Integer addition is associative, so the counter
// does not depend on the order of the waves either.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_term.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

constexpr int WAVE = 64;
static_assert(TERM_BLOCK % WAVE == 0, "whole waves");

__global__ void __launch_bounds__(TERM_BLOCK) k_term_reset(double *rec, int *cnt, int *flags, int *open, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * TERM_BLOCK + threadIdx.x;
  if (c == 0) *open = (int)n;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
  rec[TM_STATE * n + c] = (double)TERM_OPEN;
  rec[TM_DONE_STEP * n + c] = 0.0;
  rec[TM_REASON * n + c] = 0.0;
  rec[TM_SOC_DONE * n + c] = NaN;
  rec[TM_U_DONE * n + c] = NaN;
  rec[TM_T_DONE * n + c] = NaN;
  rec[TM_REST * n + c] = 0.0;
  rec[TM_STEPS * n + c] = 0.0;
  cnt[c] = 0;
  cnt[n + c] = 0;
  flags[c] = 0;
  flags[n + c] = 0;
}

__global__ void __launch_bounds__(TERM_BLOCK) k_term_seed(const double *rec, int *flag, int64_t n, int series) {
  const int64_t c = (int64_t)blockIdx.x * TERM_BLOCK + threadIdx.x;
  if (c >= n) return;
  if (rec[TM_STATE * n + c] == (double)TERM_LATCHED) flag[c / series] = 1;
}

__global__ void __launch_bounds__(TERM_BLOCK) k_term(KTerm q) {
  const int64_t n = q.n, c = (int64_t)blockIdx.x * TERM_BLOCK + threadIdx.x;
  const bool live = c < n;
  bool closed = false;
  if (live) {
    double *R = q.rec + c;
    const int64_t g = c / q.series;
    int st = (int)R[TM_STATE * n];
    const double u = q.uk[c];
    if (st == TERM_OPEN) {
      const double t = R[TM_STEPS * n] + 1.0;  // an OPEN cell was evaluated in every step since begin
      R[TM_STEPS * n] = t;
      const double z = q.soc[c], T = q.Tc[c];
      int reason = 0;
      if (z != z || u != u) {
        st = TERM_DEAD;
        R[TM_DONE_STEP * n] = t;
      } else if (q.flag_in && q.flag_in[g]) {
        reason = TERM_R_STRING;
      } else {
        const double it = q.par[TMP_I_TAPER * n + c], au = __builtin_fabs(u);
        int armed = q.cnt[c], run = q.cnt[n + c];
        if (au > it) {
          armed = 1;
          run = 0;
        } else if (armed && au <= it) {
          run += 1;
        } else {
          run = 0;
        }
        q.cnt[c] = armed;
        q.cnt[n + c] = run;
        reason = (z >= q.par[TMP_SOC_STOP * n + c] ? TERM_R_SOC : 0) | (run >= q.hold ? TERM_R_TAPER : 0) |
                 (T >= q.par[TMP_T_CUT * n + c] ? TERM_R_TEMP : 0);
      }
      if (reason) {
        st = TERM_LATCHED;
        R[TM_DONE_STEP * n] = t;
        R[TM_REASON * n] = (double)reason;
        R[TM_SOC_DONE * n] = z;
        R[TM_U_DONE * n] = u;
        R[TM_T_DONE * n] = T;
      }
      closed = st != TERM_OPEN;
      if (closed) R[TM_STATE * n] = (double)st;
    }
    if (st == TERM_LATCHED) {
      if (q.flag_out) q.flag_out[g] = 1;
      if (u == u) {  // a NaN command is left alone, as k_pack leaves it
        q.uk[c] = 0.0;
        q.uk_1[c] = 0.0;
        if (q.u) q.u[c] = 0.0;
        R[TM_REST * n] = R[TM_REST * n] + 1.0;
      }
    }
  }
  // every lane of the wave is here: the cells this wave closed, subtracted once
  const int nclosed = __popcll(__ballot(closed));
  if ((threadIdx.x & (WAVE - 1)) == 0 && nclosed) atomicAdd(q.open, -nclosed);
}

}  // namespace

static unsigned term_grid(int64_t n) { return (unsigned)((n + TERM_BLOCK - 1) / TERM_BLOCK); }

int launch_term_reset(double *rec, int *cnt, int *flags, int *open, int64_t n, void *stream) {
  hipLaunchKernelGGL(k_term_reset, dim3(n > 0 ? term_grid(n) : 1u), dim3(TERM_BLOCK), 0, (hipStream_t)stream, rec, cnt,
                     flags, open, n);
  return (int)hipGetLastError();
}

int launch_term_seed(const double *rec, int *flag, int64_t n, int series, void *stream) {
  if (n <= 0 || series < 1) return 0;
  hipLaunchKernelGGL(k_term_seed, dim3(term_grid(n)), dim3(TERM_BLOCK), 0, (hipStream_t)stream, rec, flag, n, series);
  return (int)hipGetLastError();
}

int launch_term(const KTerm &q, void *stream) {
  if (q.n <= 0 || q.series < 1) return 0;
  hipLaunchKernelGGL(k_term, dim3(term_grid(q.n)), dim3(TERM_BLOCK), 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}

}  // namespace mk
