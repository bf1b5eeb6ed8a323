// mpcekf_switch.hip -- the Np = 5 / Nc = 2 MPC step with a constraint block switched off
// (initMPC.m opts.constraints, constraintsMPC.m:18-20).
//
// A context with every switch on runs mpcekf_kernels.hip's k_cell / k_hild / k_hild_slow.
// One with a switch off splits the step the way the wide horizons do: k_cell<P_EKF | P_LIN>
// (plant, iterEKF, EKFmatsHandler; the 35-double linearisation record and zk(end)), then
//   k_mpc_sw<SW>        iterMPC.m:17-66 per cell on the enabled rows (mpc_setup<.., SW>): the
//                       problem record and hflag, or the finished cell when no QP is needed
//   k_hild_sw<SW>       hildreth.m's fast rank-2 sweep over the enabled rows (hild_cell<SW>)
//   k_hild_slow_sw<SW>  the exact-rule finisher of the lanes it flagged
// A context with per-cell limits (mpcekf_set_limits) takes the same route under every mask, 7
// included, with k_mpc_pc<SW> in k_mpc_sw's place: the same body on the cell's own limits.
// SW is a template argument: a disabled row is absent from every unrolled row loop, so the
// row number stays a constant of the loop (structural zeros, register-held constant rows,
// the LDS prefetch ring) and no sum sees a term of a disabled block.  Arithmetic follows
// orc_constraints / orc_hildreth on the compact stack, bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "mpcekf_hild.hpp"
#include "mpcekf_kernels.hpp"
#include "mpcekf_mpc.hpp"

#pragma clang fp contract(off)

namespace mk {

// iterMPC.m:17-66 and, without a QP, :75-95 -- k_cell's MPC tail on the linearisation record
template <int SW>
__global__ void __launch_bounds__(256) k_mpc_sw(const KCfg cf, const KState s, const KIO io) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = s.n;
  if (c >= n) return;
#include "mpcekf_mpc_sw.inc"
}

// k_mpc_sw with the cell's own limits (mpcekf_set_limits): lim [NLIMK][n] overlaid on a
// lane-local copy of the scalars (cfg_cell), the same body.  SW = 7 too: a per-cell context
// with every switch on takes this split route, and its record / hflag are what k_cell hands
// k_hild / k_hild_slow.
template <int SW>
__global__ void __launch_bounds__(256) k_mpc_pc(const KCfg cfs, const KState s, const KIO io, const double *lim) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = s.n;
  if (c >= n) return;
  const KCfg cf = cfg_cell(cfs, lim, n, c);
#include "mpcekf_mpc_sw.inc"
}

template <int SW>
__global__ void __launch_bounds__(256) k_hild_sw(const KCfg cf, const KState s, const KIO io) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= s.n) return;
  hild_cell<SW>(cf, s, io, c);
}

// one wave per block over a grid-stride range of waves, gone at once when k_hild_sw counted none
template <int SW>
__global__ void __launch_bounds__(64) k_hild_slow_sw(const KCfg cf, const KState s, const KIO io) {
  if (__builtin_amdgcn_readfirstlane(*s.hslow) == 0) return;
  for (int64_t w = blockIdx.x; w * 64 < s.n; w += gridDim.x) hild_slow_cell<SW>(cf, s, io, w * 64 + threadIdx.x);
}

// context-free constraintsMPC.m: the compact stack [n][nC][Nc], [n][nC] in the reference's row order
template <int SW>
__global__ void __launch_bounds__(64) k_constraints_sw(const KCfg cf, int64_t n, const double *lin,
                                                       const double *uk_1, const double *soc_k1, double *Mo,
                                                       double *go) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  constexpr int NCS = NCON_SW<SW>;
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
  constraints_s<NP, NC, SW>(cf, L, dx, uk_1[c], soc_k1[c], Phis, Hs, Cn);
#pragma unroll
  for (int ci = 0; ci < NCS; ++ci) {
    const int i = row_full<NP, NC, SW>(ci);
    go[c * NCS + ci] = Cn.gam[i];
#pragma unroll
    for (int j = 0; j < NC; ++j) Mo[(c * NCS + ci) * NC + j] = mval(Cn, i, j);
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }

// f(std::integral_constant<int, sw>) for sw = 0..6, and 7 where the caller has an all-on form
// (ALL: the per-cell k_mpc_pc)
template <bool ALL = false, class F>
static int with_sw(int sw, F &&f) {
  if constexpr (ALL) {
    if (sw == 7) {
      f(std::integral_constant<int, 7>{});
      return 0;
    }
  }
  switch (sw) {
    case 0: f(std::integral_constant<int, 0>{}); return 0;
    case 1: f(std::integral_constant<int, 1>{}); return 0;
    case 2: f(std::integral_constant<int, 2>{}); return 0;
    case 3: f(std::integral_constant<int, 3>{}); return 0;
    case 4: f(std::integral_constant<int, 4>{}); return 0;
    case 5: f(std::integral_constant<int, 5>{}); return 0;
    case 6: f(std::integral_constant<int, 6>{}); return 0;
    default: return -1;
  }
}

int launch_mpc_sw(int sw, const KCfg &c, const KState &s, const KIO &io, void *stream, const double *lim) {
  if (s.n == 0) return 0;
  const int block = spread_block(s.n, 1, 256);
  if (lim) {
    if (with_sw<true>(sw, [&](auto m) {
          hipLaunchKernelGGL(k_mpc_pc<decltype(m)::value>, dim3(grid_for(s.n, block)), dim3(block), 0,
                             (hipStream_t)stream, c, s, io, lim);
        }))
      return -1;
    return (int)hipGetLastError();
  }
  if (with_sw(sw, [&](auto m) {
        hipLaunchKernelGGL(k_mpc_sw<decltype(m)::value>, dim3(grid_for(s.n, block)), dim3(block), 0,
                           (hipStream_t)stream, c, s, io);
      }))
    return -1;
  return (int)hipGetLastError();
}

int launch_cl_diag_pc(const KCfg &c, int64_t n, const double *lin, const double *uk1, double *poles, double *sv,
                      void *stream, const double *lim) {
  if (n == 0) return 0;
  hipLaunchKernelGGL((k_cl_diag_pc<NP, NC>), dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, c, n, lin, uk1,
                     poles, sv, lim);
  return (int)hipGetLastError();
}

int launch_hild_sw(int sw, const KCfg &c, const KState &s, const KIO &io, void *stream) {
  if (s.n == 0) return 0;
  static_assert(4 * HILD_LDS_PER_WAVE <= 160 * 1024, "Hildreth slots exceed the LDS");
  const int block = spread_block(s.n, 1, 256);
  const int gs = grid_for(s.n, 64) < 256 ? grid_for(s.n, 64) : 256;
  if (with_sw(sw, [&](auto m) {
        constexpr int SW = decltype(m)::value;
        static bool attr = false;  // one per instantiation
        if (!attr) {
          (void)hipFuncSetAttribute((const void *)k_hild_sw<SW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024);
          attr = true;
        }
        hipLaunchKernelGGL(k_hild_sw<SW>, dim3(grid_for(s.n, block)), dim3(block), block / 64 * HILD_LDS_PER_WAVE,
                           (hipStream_t)stream, c, s, io);
        hipLaunchKernelGGL(k_hild_slow_sw<SW>, dim3(gs), dim3(64), HILD_LDS_PER_WAVE, (hipStream_t)stream, c, s, io);
      }))
    return -1;
  return (int)hipGetLastError();
}

int launch_constraints_sw(int sw, const KCfg &c, int64_t n, const double *lin, const double *uk_1,
                          const double *soc_k1, double *M, double *gam, void *stream) {
  if (n == 0) return 0;
  if (with_sw(sw, [&](auto m) {
        hipLaunchKernelGGL(k_constraints_sw<decltype(m)::value>, dim3(grid_for(n, 64)), dim3(64), 0,
                           (hipStream_t)stream, c, n, lin, uk_1, soc_k1, M, gam);
      }))
    return -1;
  return (int)hipGetLastError();
}

}  // namespace mk
