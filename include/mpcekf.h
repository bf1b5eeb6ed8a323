/*
 * mpcekf.h -- C-ABI of the MI355X batched MPC+EKF fast-charge control step.
 *
 * Drop-in boundary for the per-timestep loop of Rodrigops27/MPC-EKF4FastCharge
 * (runMPC.m:83-112).  The reference has no FFI of its own: its public surface
 * is the set of MATLAB functions runMPC.m calls by name.  Each entry point below
 * replaces one of them, batched over independent cells:
 *
 *   mpcekf_plant_step   <- [Vcell,obs,cellState] = OB_step(Iapp,Tc,cellState,ROM)  OB_step.m:1
 *   mpcekf_plant_step_obs  the same with every field of obs (OB_step.m:226-228,289-356)
 *   mpcekf_ekf_step     <- [zk,boundzk,ekfData,Xind] = iterEKF(vk,ik,Tk,ekfData)    iterEKF.m:30
 *   mpcekf_linearize    <- [MPC,xhat] = EKFmatsHandler(ekfData,Xind,zk,Tk)         EKFmatsHandler.m:1
 *   mpcekf_predmat      <- [Phi,G,aug] = predMat(A,B,C,D,Np,Nc)                    predMat.m:1
 *   mpcekf_constraints  <- [M,gamma] = constraintsMPC(x_aug_k,cellState,mpcData)   constraintsMPC.m:1
 *   mpcekf_mpc_step     <- [uk,mpcData] = iterMPC(xk,cellState,mpcData)            iterMPC.m:1
 *   mpcekf_hildreth     <- [DU,lambda,nexec] = hildreth(E,F,M,gamma,lambda0,maxIter) hildreth.m:1
 *   mpcekf_init_cells   <- initKF.m:30, initMPC.m:29, first OB_step call (runMPC.m:20,52,74)
 *   mpcekf_step         <- the fused loop body runMPC.m:84-111, nsteps times
 *   mpcekf_step_ex      <- the same, with every runMPC.m store (zkEst, zkBound, x_store,
 *                          mpcData.cost) per step
 *   mpcekf_step_ex_obs  <- the same, plus selected fields of OB_step's obs per step
 *
 * Conventions
 *  - Plain C types only; no exceptions cross the ABI.  Every function returns an
 *    int status (MPCEKF_OK == 0); on failure mpcekf_last_error() returns a
 *    thread-local message.
 *  - Batched arrays are cell-major ("[ncells][k]") unless stated; trajectories
 *    are step-major "[nsteps][ncells]".  All floating point is IEEE fp64.
 *  - Host pointers unless the argument is documented as "device".  Every call
 *    synchronises its HIP stream before returning.
 *  - Per-cell soft failures never fail a call: they set bits in the per-cell
 *    status word (MPCEKF_ST_*), after which that cell's outputs are NaN.  This
 *    replaces the MATLAB errors/NaN lock-out of iterEKF.m:55-59,384-389.
 *  - One context = one GPU + one HIP stream; use one host thread per context.
 *    Multi-GPU runs create one context per device on disjoint cell ranges.
 */
#ifndef MPCEKF_H
#define MPCEKF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCEKF_ABI_VERSION 5

/* return codes */
#define MPCEKF_OK 0
#define MPCEKF_E_ARG -1         /* bad argument / size                                  */
#define MPCEKF_E_ROM -2         /* ROM fails the initKF/iterEKF/OB_step structure checks */
#define MPCEKF_E_HIP -3         /* HIP runtime error                                     */
#define MPCEKF_E_UNSUPPORTED -4 /* configuration not built into this library             */
#define MPCEKF_E_STATE -5       /* call order (e.g. step before init_cells)              */

/* per-cell status bits */
#define MPCEKF_ST_ERROR 1      /* cell stopped; outputs NaN from here on                       */
#define MPCEKF_ST_LOCKOUT 2    /* warnCount > max_warn at iterEKF entry (iterEKF.m:55-59)      */
#define MPCEKF_ST_THETAE_NEG 4 /* thetae < 0 in getVariables; MATLAB errors (iterEKF.m:384-389) */

/* tfData.names codes (tf_code[] of mpcekf_rom) */
enum {
  MPCEKF_TF_negIfdl = 0, MPCEKF_TF_posIfdl, MPCEKF_TF_negIf, MPCEKF_TF_posIf, MPCEKF_TF_negIdl,
  MPCEKF_TF_posIdl, MPCEKF_TF_negPhis, MPCEKF_TF_posPhis, MPCEKF_TF_negPhise, MPCEKF_TF_posPhise,
  MPCEKF_TF_negThetass, MPCEKF_TF_posThetass, MPCEKF_TF_negPhie, MPCEKF_TF_sepPhie,
  MPCEKF_TF_posPhie, MPCEKF_TF_negThetae, MPCEKF_TF_sepThetae, MPCEKF_TF_posThetae,
  MPCEKF_TF_COUNT
};

/* The fields of OB_step's obs struct (OB_step.m:226-228, 289-356), in the order of one
 * observable record (mpcekf_obs_layout).  A vector field is as long as tfData.names says
 * (possibly 0), its entries in ROM row order (MATLAB's find); Phie has numel(ind.Phie) + 1
 * entries, -negPhise0 first (OB_step.m:320-322). */
enum {
  MPCEKF_OBS_negSOC = 0, MPCEKF_OBS_posSOC, MPCEKF_OBS_cellSOC,
  MPCEKF_OBS_negIfdl, MPCEKF_OBS_posIfdl, MPCEKF_OBS_negIfdl0, MPCEKF_OBS_posIfdl3,
  MPCEKF_OBS_negIf, MPCEKF_OBS_posIf, MPCEKF_OBS_negIf0, MPCEKF_OBS_posIf3,
  MPCEKF_OBS_negIdl, MPCEKF_OBS_posIdl,
  MPCEKF_OBS_negThetass, MPCEKF_OBS_posThetass, MPCEKF_OBS_negThetass0, MPCEKF_OBS_posThetass3,
  MPCEKF_OBS_negPhise, MPCEKF_OBS_posPhise, MPCEKF_OBS_negPhise0,
  MPCEKF_OBS_Phie, MPCEKF_OBS_Thetae,
  MPCEKF_OBS_negPhis, MPCEKF_OBS_posPhis,
  MPCEKF_OBS_Vcell,
  MPCEKF_OBS_COUNT
};

/* One electrode's cellData.function.{neg,pos} handles in tabulated form.
 * The 2-D tables are [ntemp][ntheta] (row j = the handle at T = rom.tab_T_K[j] over a
 * uniform theta grid on [0, 1]) and are evaluated by the defined bilinear interpolation
 * (theta clamped to [0, 1], T clamped to the grid ends; ntemp == 1: theta only).
 * ABI v3 (rom.tab_npoly = 4 or 6): each row is instead a piecewise polynomial in theta,
 * *_p [ntemp][ntheta-1][tab_npoly] (Uocp1_p [ntheta-1][tab_npoly]): on interval i of the
 * grid, with s = theta (ntheta-1) - i in [0, 1], c0 + s (c1 + s (... + s c_last)) (the
 * exporter fits Hermite cubics / quintics to the handles' values and theta-derivatives);
 * the node tables above stay required (the v2 route and the checks read them).  Ea[f]
 * != 0 multiplies function f (EF order Uocp, dUocp, k0, Rf, Cdleff), after the T
 * interpolation, by its Arrhenius factor exp(Ea/R (1/Tref - 1/T)) with the call's T
 * (unclamped); its rows then hold f / that factor.  So a handle k(th)exp(Ea/R(1/Tref - 1/T))
 * is exact in T, an OCP U0(th) + (T - Tref) dUdT(th) is exact in T between table rows:
 *   soc(z,T)     = soc0(T) + z*(soc100(T) - soc0(T))   iterEKF.m:282-283,439-440,497-498;
 *                                                      EKFmatsHandler.m:57-58; OB_step.m:64-65
 *   Uocp(th,T)   = Uocp       OB_step.m:313-314,337-338; iterEKF.m:362-363,404-405; EKFmatsHandler.m:84-85
 *   Uocp(th)     = Uocp1      the one-argument call, EKFmatsHandler.m:96
 *   dUocp(th,T)  = dUocp      OB_step.m:231-232; iterEKF.m:495-496,579-580
 *   k0(th,T)     = k0         OB_step.m:329-330; iterEKF.m:392-393,463-464; EKFmatsHandler.m:60-61
 *   Rf(th,T)     = Rf         OB_step.m:339-340; iterEKF.m:406-407,441-442; EKFmatsHandler.m:68-69
 *   Cdl(th,T)^(2-nDL) * wDL(th,T)^(nDL-1) = Cdleff, read at th = SOC0n/p (OB_step.m:212-219)
 * theta0/theta100 are the zero-argument calls the plant makes (OB_step.m:207-210). */
typedef struct {
  double theta0, theta100;
  const double *soc0, *soc100;                 /* [ntemp] soc(0,T), soc(1,T)       */
  const double *Uocp, *dUocp, *k0, *Rf, *Cdleff; /* [ntemp][ntheta] each            */
  const double *Uocp1;                         /* [ntheta]                         */
  /* ABI v3: theta polynomials of the same functions (NULL when tab_npoly == 0) */
  const double *Uocp_p, *dUocp_p, *k0_p, *Rf_p, *Cdleff_p; /* [ntemp][ntheta-1][tab_npoly] */
  const double *Uocp1_p;                                   /* [ntheta-1][tab_npoly]        */
  double Ea[5];            /* J/mol: Arrhenius factor of Uocp, dUocp, k0, Rf, Cdleff; 0 = none */
  /* ABI v4 (tab_npoly != 0): a function on its own theta nodes -- a lookup-table handle
   * (interp1 / pchip over measured breakpoints, which no uniform-grid polynomial follows
   * across a slope break).  Index f: Uocp, dUocp, k0, Rf, Cdleff, Uocp1.  nnode[f] = 0: the
   * uniform-grid *_p above; m = nnode[f] >= 2: node[f] [m] strictly ascending (interior nodes
   * in (0, 1)) and node_p[f] [ntemp][m-1][tab_npoly] (Uocp1: [m-1][tab_npoly]), segment k's
   * polynomial in d = theta - node[f][k]: theta clamped to [0, 1], k = #{j in 1..m-2 :
   * node[f][j] <= theta} (the end segments extend past the end nodes), then Horner and the
   * temperature blend and Arrhenius factor as for v3.  The uniform *_p of such a function may
   * be NULL.  An interp1-linear row is (y_k, slope_k, 0, 0): the handle's value to rounding. */
  int32_t nnode[6];
  const double *node[6];
  const double *node_p[6];
} mpcekf_electrode;

/* The ROM struct of runMPC.m:5 as plain arrays.  Set-points ascending. */
typedef struct {
  int32_t nT, nZ;          /* ROMmdls is nT x nZ                                  */
  int32_t n;               /* transient states per model (must be 5)               */
  int32_t nz;              /* outputs per model                                    */
  const double *T_degC;    /* xraData.T   [nT]                                     */
  const double *SOC_pct;   /* xraData.SOC [nZ]                                     */
  double Ts;               /* xraData.Tsamp                                        */
  const double *A;         /* [nT][nZ][n+1]      diag(ROMmdls(t,z).A), last == 1   */
  const double *C;         /* [nT][nZ][nz][n+1]  ROMmdls(t,z).C (with res0 column) */
  const double *D;         /* [nT][nZ][nz]       ROMmdls(t,z).D                    */
  const int32_t *tf_code;  /* [nz] MPCEKF_TF_*   tfData.names                      */
  const double *tf_xloc;   /* [nz]               tfData.xLoc                       */
  double F, R, Q, Rc, Tref;
  int32_t tab_ntheta;      /* theta grid points of the electrode tables (>= 2)     */
  int32_t tab_ntemp;       /* temperature grid points (>= 1)                       */
  const double *tab_T_K;   /* [tab_ntemp] ascending, Kelvin                        */
  int32_t tab_npoly;       /* ABI v3: 0 = linear tables; 4 / 6 = cubic / quintic *_p (and v4 node_p) */
  mpcekf_electrode neg, pos;
} mpcekf_rom;

/* also compute boundzk (iterEKF.m:186-205): on every step of a fused call that asks for a zbk
 * trajectory, otherwise on the call's last step only (what mpcekf_get_zk returns) */
#define MPCEKF_CF_BOUNDS 1

/* Controller/estimator configuration (runMPC.m:8-50, initMPC.m). */
typedef struct {
  int32_t Np, Nc;          /* horizons (runMPC.m:28-29)                          */
  double target_soc;       /* mpcData.ref, percent (runMPC.m:30)                 */
  double Crate;            /* u_min = -Q*Crate (initMPC.m:66-67)                 */
  double u_max, du_min, du_max, v_min, v_max, phise_min, z_max, z_tol;
  /* constraint switches (initMPC.m opts.constraints, constraintsMPC.m:18-20; runMPC.m:33 sets
   * all three).  Non-zero = on.  Np = 5 / Nc = 2 takes any combination; Np = 20 / Nc = 10
   * needs all three on (else MPCEKF_E_UNSUPPORTED).  The enabled blocks are stacked in the
   * reference's order, [Cu; -Cu; I; -I] (4 Nc rows), G_v (Np), -G_e (Np), then always G_soc
   * (Np): nC = (cur ? 4 Nc : 0) + (v ? Np : 0) + (eta ? Np : 0) + Np rows. */
  int32_t use_current, use_voltage, use_eta;
  int32_t max_hild;        /* mpcData.maxHild (initMPC.m:47)                     */
  double hild_tol;         /* hildreth.m:39 (1e-6)                               */
  double SigmaV, SigmaW;   /* runMPC.m:18-19                                     */
  double SigmaX0[6];       /* diagonal of SigmaX0 (runMPC.m:17)                  */
  int32_t max_warn;        /* lock-out threshold (iterEKF.m:55: > 10)            */
  int32_t flags;           /* MPCEKF_CF_*                                        */
  int32_t method;          /* initKF.m:44-49 blend: MPCEKF_METHOD_OB (runMPC.m) or _MB */
} mpcekf_config;

#define MPCEKF_METHOD_OB 0 /* output blend: every local model filtered (iterEKF.m 'OB')      */
#define MPCEKF_METHOD_MB 1 /* model blend: one blended model per cell (iterEKF.m:90-102 'MB') */

/* Layout of one linearisation record (EKFmatsHandler outputs), doubles: */
#define MPCEKF_LIN_A 0     /* [6] diag(A)              */
#define MPCEKF_LIN_CSOC 6  /* [6] Csoc                 */
#define MPCEKF_LIN_DSOC 12 /* Dsoc                     */
#define MPCEKF_LIN_CV 13   /* [6] [Cv 0]               */
#define MPCEKF_LIN_DV 19   /* Dv                       */
#define MPCEKF_LIN_CPHI 20 /* [6] [Cphi 0]             */
#define MPCEKF_LIN_DPHI 26 /* Dphi                     */
#define MPCEKF_LIN_BV 27   /* bv                       */
#define MPCEKF_LIN_BPHI 28 /* bphi                     */
#define MPCEKF_LIN_XHAT 29 /* [6] xhat (model + 0)     */
#define MPCEKF_LIN_SIZE 35

typedef struct mpcekf_ctx mpcekf_ctx;

int mpcekf_abi_version(void);
/* sha256 prefix of the sources this library was built from (profiles record the one
 * they were measured on; bench.py refuses stale PMC figures). */
const char *mpcekf_build_id(void);
const char *mpcekf_last_error(void);
void mpcekf_config_defaults(mpcekf_config *cfg); /* the runMPC.m values */

/* Context: owns the device copy of the ROM and the per-cell state (SoA/AoS in HBM). */
int mpcekf_ctx_create(const mpcekf_rom *rom, const mpcekf_config *cfg, int device, int64_t ncells,
                      mpcekf_ctx **out);
int mpcekf_ctx_destroy(mpcekf_ctx *ctx);
/* ncon: nC of the configuration's constraint switches (23 at Np = 5 / Nc = 2 with all on). */
int mpcekf_ctx_info(const mpcekf_ctx *ctx, int64_t *ncells, int32_t *nmodels, int32_t *nz, int32_t *ncon);
/* The configuration the context was created with (e.g. its method, for a checkpoint). */
int mpcekf_ctx_config(const mpcekf_ctx *ctx, mpcekf_config *cfg);

/* initKF + initMPC + OB_step first call for every cell: SOC0 in percent, Tc in degC
 * (the cell temperature until a call passes another one). */
int mpcekf_init_cells(mpcekf_ctx *ctx, const double *soc0_pct, const double *tc_degC);

/* nsteps fused closed-loop steps.  tc_degC is the temperature runMPC.m:85-92 passes to
 * OB_step, iterEKF and EKFmatsHandler at each step, [nsteps][ncells] in degC, or NULL to
 * keep every cell's current temperature.  Each output may be NULL; non-NULL outputs are
 * [nsteps][ncells] host arrays (or device arrays when outputs_on_device != 0, which
 * then also applies to tc_degC):
 *   traj_u = u_store (MPC command), traj_v = voltage_store, traj_soc = SOC_store
 *   (zk(end)), traj_phise = phise_store, traj_nexec = mpcData.cost.nexec. */
int mpcekf_step(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, double *traj_u, double *traj_v,
                double *traj_soc, double *traj_phise, int32_t *traj_nexec, int32_t outputs_on_device);

/* Per-step outputs of mpcekf_step_ex (runMPC.m:55-69 stores, filled at runMPC.m:94-111
 * and iterMPC.m:89-95).  Every pointer may be NULL.  Step-major arrays, host pointers
 * (device pointers when outputs_on_device != 0):
 *   [nsteps][ncells]       u, v, soc, phise, nexec, J_unc, J_fin, norm_du, nviol
 *   [nsteps][ncells][6]    x    (x_store: the EKFmatsHandler xhat, integrator state last)
 *   [nsteps][ncells][nz+2] zk, zbk (zkEst / zkBound; zbk needs MPCEKF_CF_BOUNDS)
 *   [nsteps][ncells][7][2] poles (mpcData.poles = eig(CL), iterMPC.m:53-59: re, im;
 *                          sorted by descending real, then imaginary part)
 *   [nsteps][ncells][7]    sv    (mpcData.sv = svd(CL), iterMPC.m:60, descending)
 * A cell in error has NaN floating outputs and zero nexec / nviol from its failing step on. */
typedef struct {
  double *u, *v, *soc, *phise;     /* u_store, voltage_store, SOC_store, phise_store    */
  int32_t *nexec;                  /* mpcData.cost.nexec                                */
  double *x;                       /* x_store                                           */
  double *zk, *zbk;                /* zkEst, zkBound                                    */
  double *J_unc, *J_fin, *norm_du; /* mpcData.cost.J_uncon / J_final / norm_DU          */
  int32_t *nviol;                  /* mpcData.cost.viol                                 */
  double *poles, *sv;              /* mpcData.poles, mpcData.sv (stability diagnostics) */
} mpcekf_traj;
int mpcekf_step_ex(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                   int32_t outputs_on_device);

/* mpcekf_step_ex plus the plant's observables of every step: obs [nsteps][nslots][ncells]
 * (host, or device when outputs_on_device != 0), slot s of the record of mpcekf_obs_layout at
 * position p = its index in slots[]; duplicates allowed.  Row k is OB_step's obs of step k:
 * the plant's own values (obs.negPhise0 is the plant's side-reaction overpotential, where
 * traj.phise is the EKF's estimate), bit for bit what mpcekf_plant_step_obs gives for the same
 * state, current and temperature.  A cell with MPCEKF_ST_ERROR at the start of a step has NaN
 * in that step's row.  nslots == 0 (slots, obs NULL) is mpcekf_step_ex.  MPCEKF_E_ARG: a slot
 * outside 0..nobs-1, nslots < 0, a NULL among slots/obs with nslots > 0. */
int mpcekf_step_ex_obs(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                       const int32_t *slots, int32_t nslots, double *obs, int32_t outputs_on_device);

/* Optional per-step EKF output of the LAST mpcekf_step call: zk and boundzk
 * ([ncells][nz+2], boundzk only with MPCEKF_CF_BOUNDS) of that call's last step.  A fused call
 * of several steps evaluates boundzk (and stores zk) on every step only when it is given their
 * trajectory (mpcekf_traj.zbk / .zk); otherwise it evaluates them on its last step alone, the
 * only one this getter can return.  A call of one step evaluates them as ever. */
int mpcekf_get_zk(mpcekf_ctx *ctx, double *zk, double *boundzk);

/* eig / svd of one n x n (n <= 8) row-major matrix on the host, as the fused step
 * computes mpcData.poles / mpcData.sv (iterMPC.m:57-60): re/im sorted by descending real
 * then imaginary part, sv descending; any output may be NULL.  Returns MPCEKF_E_ARG for
 * n outside 1..8; non-finite input gives NaN outputs. */
int mpcekf_cl_eig(int32_t n, const double *a, double *re, double *im, double *sv);

/* ---- stage entry points (one MATLAB function each; all batched over cells) ----
 * Each has an _async twin with the same arguments ("every call returns
 * after hipStreamSynchronize unless _async is used"): it enqueues the call's copies and
 * kernels on the context's stream in order and returns without waiting.  Host inputs are
 * copied before it returns (the caller may free or reuse them; an input above
 * MPCEKF_BOUNCE_MAX bytes is read in place and must stay alive until the synchronisation).
 * Host outputs are written by the time mpcekf_sync(ctx) or the next synchronous stage call
 * returns -- not before; the caller keeps those arrays alive and unread until then.  Errors
 * of the enqueued copies are reported by that synchronisation.  The synchronous calls copy
 * outputs in chunks whose DMA overlaps the host-side copy (a worker pool, MPCEKF_CHUNK bytes
 * per chunk, MPCEKF_COPY_THREADS workers).
 * The temperature argument (Tc of OB_step.m:1, Tk of iterEKF.m:30 / EKFmatsHandler.m:1,
 * degC, [ncells]) sets each cell's temperature for this and later calls; NULL keeps it. */
/* OB_step: applies iapp[c] to the plant state at tc_degC[c], returns vcell[c] (may be NULL:
 * Vcell also stays on the device for the next mpcekf_ekf_step with vk = NULL). */
int mpcekf_plant_step(mpcekf_ctx *ctx, const double *iapp, const double *tc_degC, double *vcell);
/* Slot offsets of the observable record: field f (MPCEKF_OBS_*) occupies slots off[f] ..
 * off[f + 1] - 1, off[MPCEKF_OBS_COUNT] = nobs, the record length. */
int mpcekf_obs_layout(const mpcekf_ctx *ctx, int32_t off[MPCEKF_OBS_COUNT + 1]);
/* OB_step with its obs output: mpcekf_plant_step's contract (the same Vcell and plant state,
 * bit for bit) plus the observable record of this step, obs [nobs][ncells] (slot-major: each
 * slot one contiguous per-cell vector).  obs may be NULL: the record stays on the device for
 * mpcekf_plant_obs_slots.  A cell with MPCEKF_ST_ERROR has NaN in every slot.  The record's
 * device memory is allocated by the first call. */
int mpcekf_plant_step_obs(mpcekf_ctx *ctx, const double *iapp, const double *tc_degC, double *vcell, double *obs);
/* Selected slots of the device-resident record of the last mpcekf_plant_step_obs: out
 * [nslots][ncells] (8 bytes per cell and slot cross PCIe, not 8 nobs).  MPCEKF_E_STATE when
 * there is no record since init / the last fused step / set_state; MPCEKF_E_ARG for a slot
 * outside 0 .. nobs - 1. */
int mpcekf_plant_obs_slots(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, double *out);
/* iterEKF: zk/boundzk [ncells][nz+2], xind_model [ncells][4] (model index t*nZ+z of
 * Xind.theT/theZ), xind_gamma [ncells][4].  Every output may be NULL: zk and Xind also stay
 * on the device for the next mpcekf_linearize (runMPC.m:91 -> :94 without a host round trip).
 * vk = NULL: the last mpcekf_plant_step's Vcell on the device (MPCEKF_E_STATE without one). */
int mpcekf_ekf_step(mpcekf_ctx *ctx, const double *vk, const double *ik, const double *tk_degC, double *zk,
                    double *boundzk, int32_t *xind_model, double *xind_gamma);
/* EKFmatsHandler: lin [ncells][MPCEKF_LIN_SIZE], or NULL (the record stays on the device for
 * mpcekf_mpc_step / mpcekf_mpc_diag with lin = NULL and mpcekf_lin_fields).  zk, xind_model and
 * xind_gamma are all given, or all NULL for the device copies of the last mpcekf_ekf_step
 * (MPCEKF_E_STATE if there was none since init / the last fused step / set_state). */
int mpcekf_linearize(mpcekf_ctx *ctx, const double *zk, const int32_t *xind_model, const double *xind_gamma,
                     const double *tk_degC, double *lin);
/* Selected slots (MPCEKF_LIN_*) of the device-resident linearisation records of the last
 * mpcekf_linearize: out [ncells][nslots] (may be NULL), and set [ncells][nslots] (may be NULL)
 * written into those slots first -- e.g. runMPC.m:95-96 reads MPC.Cphi / Dphi / bphi and xhat
 * (14 doubles of the 35), and an iterMPC caller with another xk writes MPCEKF_LIN_XHAT.. */
int mpcekf_lin_fields(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, const double *set, double *out);
/* iterMPC (uses and updates the context's uk_1 and lambda warm start):
 * soc_k1 = mpcData.SOCk_1 per cell; outputs uk, nexec.  lin = NULL: the device-resident
 * record of the last mpcekf_linearize; soc_k1 = NULL: zk(end) of the last mpcekf_ekf_step on
 * the device (runMPC.m:99's mpcData.SOCk_1 = zk(end)). */
int mpcekf_mpc_step(mpcekf_ctx *ctx, const double *lin, const double *soc_k1, double *uk, int32_t *nexec);
/* The same, also returning this call's iterMPC.m:89-95 cost log (mpcData.cost.J_uncon,
 * J_final, norm_DU, viol) per cell; any of the four may be NULL. */
int mpcekf_mpc_step_ex(mpcekf_ctx *ctx, const double *lin, const double *soc_k1, double *uk, int32_t *nexec,
                       double *J_unc, double *J_fin, double *norm_du, int32_t *nviol);
/* iterMPC.m:53-60 stability analysis of the iterMPC that mpcekf_mpc_step would run on lin:
 * Kmpc = first row of E\(G_soc'*Phi_soc), CL = Abar - Bbar*Kmpc; poles [ncells][7][2]
 * (eig(CL): re, im, sorted as in mpcekf_traj), sv [ncells][7] (svd(CL)).  uk_1 [ncells]
 * (mpcData.uk_1) or NULL for the context's current one (call before mpcekf_mpc_step).
 * Reads nothing else of the context's state and changes none of it.  lin = NULL: the
 * device-resident record of the last mpcekf_linearize. */
int mpcekf_mpc_diag(mpcekf_ctx *ctx, const double *lin, const double *uk_1, double *poles, double *sv);
/* the _async twins (see above) */
int mpcekf_plant_step_async(mpcekf_ctx *ctx, const double *iapp, const double *tc_degC, double *vcell);
int mpcekf_plant_step_obs_async(mpcekf_ctx *ctx, const double *iapp, const double *tc_degC, double *vcell,
                                double *obs);
int mpcekf_plant_obs_slots_async(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, double *out);
int mpcekf_ekf_step_async(mpcekf_ctx *ctx, const double *vk, const double *ik, const double *tk_degC, double *zk,
                          double *boundzk, int32_t *xind_model, double *xind_gamma);
int mpcekf_linearize_async(mpcekf_ctx *ctx, const double *zk, const int32_t *xind_model, const double *xind_gamma,
                           const double *tk_degC, double *lin);
int mpcekf_lin_fields_async(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, const double *set, double *out);
int mpcekf_mpc_step_async(mpcekf_ctx *ctx, const double *lin, const double *soc_k1, double *uk, int32_t *nexec);
int mpcekf_mpc_step_ex_async(mpcekf_ctx *ctx, const double *lin, const double *soc_k1, double *uk, int32_t *nexec,
                             double *J_unc, double *J_fin, double *norm_du, int32_t *nviol);
int mpcekf_mpc_diag_async(mpcekf_ctx *ctx, const double *lin, const double *uk_1, double *poles, double *sv);

/* Context-free batched kernels (device chosen by `device`).
 * predMat with A = diag(a), B = ones: a,C [n][6], D [n] -> Phi [n][Np][7], G [n][Np][Nc]. */
int mpcekf_predmat(int device, int64_t n, int32_t Np, int32_t Nc, const double *a, const double *C,
                   const double *D, double *Phi, double *G);
/* constraintsMPC: lin [n][LIN], uk_1/soc_k1 [n] -> M [n][ncon][Nc], gamma [n][ncon], with
 * ncon = nC of cfg's switches: only the enabled blocks' rows, in the reference's order. */
int mpcekf_constraints(int device, const mpcekf_config *cfg, double Q, int64_t n, const double *lin,
                       const double *uk_1, const double *soc_k1, double *M, double *gamma);
/* hildreth: E [n][Nc][Nc], F [n][Nc], M [n][ncon][Nc], gamma/lambda [n][ncon]; lambda is
 * the warm start in and the multipliers out; DU [n][Nc]; nexec [n].  Any M with
 * 1 <= Nc <= 10 and 1 <= ncon <= 100 (hildreth.m:1; Nc = 2 / ncon = 23 is the compiled
 * fused-path form, other sizes a runtime-sized kernel with the same defined arithmetic). */
int mpcekf_hildreth(int device, int64_t n, int32_t Nc, int32_t ncon, const double *E, const double *F,
                    const double *M, const double *gamma, double *lambda, int32_t max_iter, double tol,
                    double *DU, int32_t *nexec);

/* hildreth.m for the constraint pattern of constraintsMPC.m as runMPC configures it
 * (Np = 5, Nc = 2, all three switches): M = [Cu; -Cu; I; -I; G_v; -G_e; G_soc] given by
 * the Toeplitz columns Hv, He, Hs [n][5] (G_v(i,j) = Hv(i-j) for j <= i).  This is the
 * solver the fused step runs (rank-2 form, hildreth.m:17-46); E [n][2][2], F [n][2],
 * gamma/lambda [n][23], DU [n][2], nexec [n] as in mpcekf_hildreth.  Always the all-on
 * pattern: a stack with a block switched off goes through mpcekf_hildreth with its compact
 * M (mpcekf_constraints). */
int mpcekf_hildreth_structured(int device, int64_t n, const double *E, const double *F, const double *Hv,
                               const double *He, const double *Hs, const double *gamma, double *lambda,
                               int32_t max_iter, double tol, double *DU, int32_t *nexec);

/* ---- instrumentation (not part of the reference interface) ---- */
/* When enabled, mpcekf_step brackets every kernel launch with HIP events on the
 * context's stream; enable = N > 1 samples steps N-1, 2N-1, ... and the last only (the
 * events then perturb the timed stream N times less; with N dividing 32 the sampled steps
 * include every flush).  mpcekf_get_timing returns the summed milliseconds and launch
 * counts of [plant, flush, cell, hild, bounds] (arrays of MPCEKF_NKERNELS) since the
 * last call and resets them.  "flush" is the all-model time update (k_flush, every
 * 32 steps and at the end of each call); "bounds" is boundzk (k_bounds, when
 * MPCEKF_CF_BOUNDS is set): its milliseconds and its launch count cover only the steps that
 * launched k_bounds, which are every step of a call with a zbk trajectory and the last step
 * of any other call. */
#define MPCEKF_K_PLANT 0
#define MPCEKF_K_FLUSH 1
#define MPCEKF_K_CELL 2
#define MPCEKF_K_HILD 3
#define MPCEKF_K_BOUNDS 4
#define MPCEKF_NKERNELS 5
int mpcekf_set_timing(mpcekf_ctx *ctx, int32_t enable);
/* Graph replay of the fused call (runMPC.m:83-112's loop as a device graph, SURVEY.md
 * §8(f) row 2): with enable != 0, mpcekf_step / mpcekf_step_ex capture each new call
 * shape (nsteps, output and temperature buffers, diagnostics) into a hipGraph once and
 * replay it on later calls of the same shape -- the per-step launches of a control loop
 * that calls mpcekf_step(ctx, 1, ...) every period become one graph launch.  Results are
 * identical; ignored while mpcekf_set_timing is on.  Also MPCEKF_GRAPH=1 at create. */
int mpcekf_set_graph(mpcekf_ctx *ctx, int32_t enable);
int mpcekf_get_timing(mpcekf_ctx *ctx, double *ms_sum, int64_t *launches);
/* The Hildreth problem records of the last fused step, as k_cell left them for
 * k_hild (field-major [MPCEKF_PROB_DOUBLES][ncells]: E(2x2) F(2) Hv(5) He(5) Hs(5)
 * gamma(23) e(5) Ru uk_1), and hflag [ncells] (1 = the QP ran).  The layout does not
 * depend on the constraint switches: gamma keeps the all-on row slots, and the fields of a
 * disabled block (its Hv / He, its gamma rows) read 0.  For replaying the solver offline
 * (tools/micro); either pointer may be NULL. */
#define MPCEKF_PROB_DOUBLES 51
int mpcekf_get_hild_problems(mpcekf_ctx *ctx, double *prob, int32_t *hflag);
/* Profiling builds only (-DMPCEKF_STAMPS, tools/stamps.py): shader-clock stamps at the
 * section boundaries of the EKF/MPC kernel (rows 0..11) and the plant kernel (rows
 * 12..19) for the last fused step, [MPCEKF_NSTAMPS][ncells].  Rows 12..19 are written
 * only when the plant runs as its own kernel (k_plant4: MPCEKF_CELL_PLANT=0 or the
 * lane-quad path); when it runs inside k_cell (the default) they read 0.  *nstamps = 0
 * (and nothing written) in normal builds.  ABI v3: 20 rows (v2 had 12). */
#define MPCEKF_NSTAMPS 20
int mpcekf_get_stamps(mpcekf_ctx *ctx, int64_t *stamps, int32_t *nstamps);

/* ---- per-cell MPC limits and targets (the charging protocol of runMPC.m:30-44 per cell) ----
 * mpcekf_config holds one targetSOC, C-rate and limits set for the whole context.  These
 * entry points give cells of one context their own: a protocol sweep (phise_min against
 * v_max against C-rate), per-cell targets in a pack.  The field ids name mpcekf_config's
 * fields, in its units. */
enum {
  MPCEKF_LIM_TARGET_SOC = 0, MPCEKF_LIM_CRATE, MPCEKF_LIM_U_MAX, MPCEKF_LIM_DU_MIN, MPCEKF_LIM_DU_MAX,
  MPCEKF_LIM_V_MAX, MPCEKF_LIM_PHISE_MIN, MPCEKF_LIM_Z_MAX, MPCEKF_LIM_Z_TOL, MPCEKF_NLIM
};
/* mpcData.ref and mpcData.const of runMPC.m:30-44 per cell: fields[nfields] are distinct
 * MPCEKF_LIM_* ids, values [nfields][ncells] (row i = field fields[i] of every cell).  A
 * field never named keeps the context's scalar.  The MPC kernels read u_min = -Q * Crate
 * (initMPC.m:66-67) and zmax = z_max + z_tol (constraintsMPC.m:90-91), formed on the host by
 * the expressions the scalar configuration goes through, so arrays constant at the
 * configuration's values give the bits of the scalar context.  May be called at any point
 * after mpcekf_ctx_create, mid-charge included; ordered on the context's stream, it takes
 * effect at the next MPC stage (the fused step, mpcekf_mpc_step(_ex)(_async), mpcekf_mpc_diag)
 * and leaves the stage route's device-resident zk / Xind / lin records valid.  No value is
 * refused (mpcekf_ctx_create checks none of these fields either).  Np = 5 / Nc = 2 takes
 * every constraint mask; Np = 20 / Nc = 10 all three switches on, as ever.  The first call
 * moves the context to the split launch sequence and retires its captured
 * graphs; later calls rewrite the same device buffer.  MPCEKF_E_ARG: a NULL pointer, nfields
 * outside 1..MPCEKF_NLIM, an unknown or repeated field id.
 * The context-free mpcekf_constraints / mpcekf_predmat / mpcekf_hildreth* keep their scalar
 * mpcekf_config. */
int mpcekf_set_limits(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, const double *values);
/* The values in force, values [nfields][ncells]: what mpcekf_set_limits stored, the
 * configuration's scalar (broadcast) for a field never set or after mpcekf_clear_limits
 * (runMPC.m:30-44 / initMPC.m:66-67 / constraintsMPC.m:90-91 in mpcekf_config's terms). */
int mpcekf_get_limits(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Back to the configuration's scalars of runMPC.m:30-44 (initMPC.m:66-67,
 * constraintsMPC.m:90-91) and to the launch sequence the context had before its first
 * mpcekf_set_limits; a no-op on a context that never set any. */
int mpcekf_clear_limits(mpcekf_ctx *ctx);

/* ---- per-cell charge summary along the fused loop (not part of the reference interface) ----
 * What a protocol sweep reads back per cell -- time to a SOC, the smallest side-reaction
 * overpotential, peak voltage and current, charge moved, solver effort -- accumulated on the
 * device over any number of calls, instead of runMPC.m:55-69's per-step stores reduced on the
 * host.  mpcekf_step_summary is mpcekf_step's fused loop (runMPC.m:84-111) with no trajectory
 * output: the same launches and the same state, bit for bit; each step's u_store,
 * voltage_store, SOC_store, phise_store and cost.nexec rows (and one slot of OB_step's obs)
 * go to a window of MPCEKF_SUM_WIN rows on the device, folded into the record once per
 * window and at the end of the call, so the call's device memory does not grow with nsteps.
 *
 * t counts the summary steps since mpcekf_summary_begin, from 1, across calls.  A step is
 * counted for a cell when none of its u, v, soc, phise is NaN (a cell in error has NaN
 * outputs from its failing step on).  Every value is a double; step indices and counts are
 * exact integers.
 *   SEEN        steps run since begin, counted or not
 *   STEPS       counted steps
 *   ERR_STEP    t of the first step not counted; 0: none
 *   T_REACH     t of the first counted step with soc >= soc_reach[c]; 0: never, or no
 *               threshold.  soc_reach is in mpcekf_traj.soc's unit: zk(end) (runMPC.m:109), the
 *               EKF's SOC as a fraction 0..1 (SOC0 / 100 - x0 Ts / (3600 Q)) -- not the
 *               percent of mpcekf_config.target_soc and mpcekf_init_cells
 *   U_MIN, U_MIN_STEP, U_MAX            over counted steps of u_store (a charging current is
 *                                       negative: U_MIN is the peak charging current)
 *   V_MAX, V_MAX_STEP, V_MIN            voltage_store
 *   PHISE_MIN, PHISE_MIN_STEP           phise_store, the EKF's estimate (runMPC.m:94-95)
 *   U_LAST, V_LAST, SOC_LAST, PHISE_LAST   the last counted step's values
 *   U_SUM       u added in step order, plain fp64 additions from +0 (Ah = -U_SUM Ts / 3600)
 *   NEXEC_SUM, NEXEC_MAX, NSAT          cost.nexec over counted steps; NSAT: steps with
 *                                       nexec >= max_hild
 *   OBS_MIN, OBS_MIN_STEP, OBS_MAX, OBS_MAX_STEP   the plant's slot obs_slot over the steps
 *               where it is not NaN (counted or not); NaN / 0 without a slot
 * An extremum is replaced only on a strict < / >: the first occurrence wins, and -0 and +0 do
 * not displace each other.  With no counted step the extrema (NEXEC_MAX too) and the _LAST
 * fields are NaN, their step fields and the sums 0. */
enum {
  MPCEKF_SUM_SEEN = 0, MPCEKF_SUM_STEPS, MPCEKF_SUM_ERR_STEP, MPCEKF_SUM_T_REACH,
  MPCEKF_SUM_U_MIN, MPCEKF_SUM_U_MIN_STEP, MPCEKF_SUM_U_MAX,
  MPCEKF_SUM_V_MAX, MPCEKF_SUM_V_MAX_STEP, MPCEKF_SUM_V_MIN,
  MPCEKF_SUM_PHISE_MIN, MPCEKF_SUM_PHISE_MIN_STEP,
  MPCEKF_SUM_U_LAST, MPCEKF_SUM_V_LAST, MPCEKF_SUM_SOC_LAST, MPCEKF_SUM_PHISE_LAST,
  MPCEKF_SUM_U_SUM, MPCEKF_SUM_NEXEC_SUM, MPCEKF_SUM_NEXEC_MAX, MPCEKF_SUM_NSAT,
  MPCEKF_SUM_OBS_MIN, MPCEKF_SUM_OBS_MIN_STEP, MPCEKF_SUM_OBS_MAX, MPCEKF_SUM_OBS_MAX_STEP,
  MPCEKF_NSUM
};
#define MPCEKF_SUM_WIN 64 /* steps per window: the rows of device scratch a summary call uses */
/* Allocates the record (first call) and resets it; soc_reach [ncells] or NULL (no threshold:
 * T_REACH stays 0); obs_slot: one slot of mpcekf_obs_layout's record (e.g. negPhise0, the
 * plant's own plating margin), or -1 for none.  A second begin resets the record.  May be
 * called before mpcekf_init_cells (which does not touch the record).  MPCEKF_E_ARG: a NULL
 * ctx, obs_slot outside -1 .. nobs - 1. */
int mpcekf_summary_begin(mpcekf_ctx *ctx, const double *soc_reach, int32_t obs_slot);
/* nsteps fused steps (mpcekf_step's, tc_degC as there: host [nsteps][ncells] or NULL) folded
 * into the record.  MPCEKF_E_STATE without a begin (or before mpcekf_init_cells);
 * MPCEKF_E_ARG: nsteps < 0.  A refused call leaves the context and the record as they were.
 * The kernel that folds a window is not one of mpcekf_set_timing's five slots. */
int mpcekf_step_summary(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_SUM_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NSUM, an unknown or repeated id. */
int mpcekf_get_summary(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the record and the window; the context then behaves as one that never began.  A
 * no-op without a begin. */
int mpcekf_summary_end(mpcekf_ctx *ctx);

/* ---- per-cell lumped thermal model along the fused loop (not part of the reference interface) ----
 * runMPC.m:85-92 passes a temperature TC it is given.  With a model, the cell temperature is a
 * state: after every fused step the library advances it on the device from the current the
 * step applied and the voltage the plant answered with, and the next step (or the next stage
 * call) reads it -- a charge with self-heating at the fused loop's speed.  Per cell, after
 * fused step t (Ts = rom.Ts), every line one or more separately rounded fp64 operations in
 * exactly this order (no contraction into fused multiply-adds, IEEE division):
 *   i    = the current OB_step applied in step t: MPCEKF_S_UK as it stood before the step
 *          (= u_store(t-1))
 *   v    = voltage_store(t): the plant's Vcell of step t (MPCEKF_S_VK); NaN for a cell that
 *          has MPCEKF_ST_ERROR after the step (its outputs are NaN from its failing step on)
 *   z    = (SOCnAvg - theta0n) / (theta100n - theta0n)      cellState.SOCnAvg after the step
 *          (MPCEKF_S_SOCNAVG); OB_step.m:228's cellSOC, the obs record's cellSOC of step t+1
 *   zc   = z > 0 ? z : 0;   zc = zc < 1 ? zc : 1            (a NaN z gives 0)
 *   s    = zc * (double)(nocv - 1);   j = min((int)s, nocv - 2);   f = s - (double)j
 *   U    = ocv[j] + f * (ocv[j+1] - ocv[j])                 open-circuit voltage over z in [0, 1]
 *   q    = i * (U - v)                                      W; charging: i < 0, v > U, q > 0
 *   loss = (T - Tamb) / Rth                                 Rth = +inf: adiabatic (loss = 0)
 *   Tn   = T + ((q - loss) * Ts) / Cth
 *   T   <- Tn if isfinite(Tn) and Tn <= 100 (the rule every temperature argument passes);
 *          otherwise T is held and NHELD counts the step
 * T is the context's cell temperature (degC): what mpcekf_init_cells or a stage call's
 * temperature argument set.  Stage calls do not advance the model; their temperature argument
 * still sets T.  Entropic (reversible) heat is not modelled.
 * The record, every value a double, counts and step indices exact integers:
 *   T            the cell temperature now
 *   T_MAX, T_MAX_STEP, T_MIN   over the temperatures the steps used (T before the update),
 *                replaced only on a strict > / <; T_MAX_STEP counts the model's steps from 1
 *                since begin, across calls.  NaN / 0 before the first step
 *   HEAT_SUM     the finite q values added in step order, plain fp64 additions from +0
 *                (energy in J = HEAT_SUM * Ts)
 *   STEPS        steps whose T was advanced
 *   NHELD        steps whose T was held */
enum { MPCEKF_TH_CTH = 0 /* J/K */, MPCEKF_TH_RTH /* K/W, +inf allowed */, MPCEKF_TH_TAMB /* degC */, MPCEKF_NTH };
enum {
  MPCEKF_THR_T = 0, MPCEKF_THR_T_MAX, MPCEKF_THR_T_MAX_STEP, MPCEKF_THR_T_MIN, MPCEKF_THR_HEAT_SUM,
  MPCEKF_THR_STEPS, MPCEKF_THR_NHELD, MPCEKF_NTHR
};
/* Gives the context a model: params [MPCEKF_NTH][ncells], the open-circuit voltage table ocv
 * [nocv] on a uniform grid of cell SOC 0..1, t0_degC [ncells] the temperature to start from or
 * NULL to keep the context's.  Allocates the model's device buffers (first call) and resets the
 * record; a second begin replaces parameters and table and resets the record.  May be called
 * before mpcekf_init_cells, which sets T as ever and does not touch the record.  From then on
 * every fused call (mpcekf_step, _step_ex, _step_ex_obs, _step_summary, _step_ex_thermal)
 * advances the model once per step and takes tc_degC == NULL only: with a tc_degC it returns
 * MPCEKF_E_ARG and leaves the context and the record as they were.  The model's kernel is not
 * one of mpcekf_set_timing's five slots.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx, params or ocv; a Cth that is not finite and > 0;
 * an Rth that is not > 0 (+inf allowed); a Tamb or t0 that is not finite and <= 100; nocv < 2;
 * a non-finite ocv entry. */
int mpcekf_thermal_begin(mpcekf_ctx *ctx, const double *params, int32_t nocv, const double *ocv,
                         const double *t0_degC);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_THR_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NTHR, an unknown or repeated id. */
int mpcekf_thermal_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the model; T stays what it is and the context then behaves as one that never began
 * (tc_degC == NULL keeps T).  A no-op without a begin. */
int mpcekf_thermal_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_obs on a thermal context plus the model's rows, [nsteps][ncells] (host, or
 * device when outputs_on_device != 0), either may be NULL: temp[t] the temperature step t
 * used, heat[t] its q (NaN for a cell in error).  MPCEKF_E_STATE without a begin. */
int mpcekf_step_ex_thermal(mpcekf_ctx *ctx, int32_t nsteps, const mpcekf_traj *traj, const int32_t *slots,
                           int32_t nslots, double *obs, double *temp, double *heat, int32_t outputs_on_device);

/* ---- the MPC limits scheduled over the model's temperature (not part of the reference interface) ----
 * runMPC.m:30-44 sets the controller's limits once.  A battery management system derates them
 * over temperature: the allowed C-rate falls as the cell warms, the plating margin rises when it
 * is cold.  A schedule is a set of tables of limit fields over a uniform temperature grid,
 * evaluated per cell on the device in every fused step, so the limits the MPC stage reads follow
 * the temperature the thermal model computes -- inside one fused call, graph replay and
 * mpcekf_step_summary included.  It goes through the existing current, voltage and eta blocks of
 * constraintsMPC.m and changes no QP structure; there is no T_max row in the stack.
 *
 * fields[nfields]: distinct ids among MPCEKF_LIM_CRATE, _U_MAX, _DU_MIN, _DU_MAX, _V_MAX,
 * _PHISE_MIN (the fields whose kernel slot is one number; TARGET_SOC, Z_MAX, Z_TOL cannot be
 * scheduled).  tables [nsets][nfields][ntab] in mpcekf_config's units: entry k of a table is the
 * field's value at T_lo + k (T_hi - T_lo) / (ntab - 1) degC.  set_of_cell [ncells] gives each
 * cell its table set 0..nsets-1 (one batch sweeps several derating maps); NULL: set 0.
 *
 * For every fused step t and every cell, the MPC stage of step t reads, for each scheduled field,
 * the table value at the temperature step t used: temp[t] of mpcekf_step_ex_thermal, the cell
 * temperature as the step finds it -- the first step of a call after mpcekf_init_cells, after a
 * mpcekf_thermal_begin with t0, or after a stage call's temperature argument included.  Fields not
 * scheduled keep what mpcekf_set_limits stored, or the configuration's scalar.  Per cell and
 * field, every line one or more separately rounded fp64 operations in exactly this order (no
 * contraction, IEEE division), the shape of the model's open-circuit voltage lookup:
 *   x   = (T - T_lo) / (T_hi - T_lo)
 *   xc  = x > 0 ? x : 0;   xc = xc < 1 ? xc : 1             (a NaN x gives 0)
 *   s   = xc * (double)(ntab - 1);   j = min((int)s, ntab - 2);   f = s - (double)j
 *   val = tab[j] + f * (tab[j+1] - tab[j])
 * The kernels' slot is formed from val by the expression the scalar configuration goes through
 * (u_min = -Q * val for CRATE, val itself for the others), so a table constant at the
 * configuration's value feeds the MPC kernels the scalar's bits.
 *
 * Needs a model: MPCEKF_E_STATE before mpcekf_thermal_begin.  Setting a schedule moves the
 * context to the per-cell launch sequence if it is not there already, and
 * evaluates the schedule once at the temperatures as they stand.  A second call replaces the
 * schedule (fields of the first that the second does not name go back to their mpcekf_set_limits
 * / configuration values); captured graphs stay valid.  While a schedule is active,
 * mpcekf_get_limits returns for a scheduled field the value in force after the last evaluation
 * (after a fused call: what its last step used); mpcekf_set_limits naming a scheduled field
 * returns MPCEKF_E_ARG and mpcekf_clear_limits returns MPCEKF_E_STATE, both changing nothing.
 * The stage route (mpcekf_mpc_step(_ex), mpcekf_mpc_diag) does not evaluate the schedule, as it
 * does not advance the model: it reads the values of the last evaluation.  The schedule's kernels
 * are not among mpcekf_set_timing's five slots.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx, fields or tables; nfields outside 1..6; a repeated
 * id or one that cannot be scheduled; ntab < 2; T_lo or T_hi not finite, or T_hi <= T_lo; a
 * non-finite table entry; nsets < 1; a set_of_cell entry outside 0..nsets-1 (the message names
 * the cell). */
int mpcekf_thermal_schedule(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, int32_t ntab, double T_lo_degC,
                            double T_hi_degC, int32_t nsets, const double *tables, const int32_t *set_of_cell);
/* Ends the schedule: its fields go back to what mpcekf_set_limits or the configuration last gave
 * them, and the launch sequence stays per-cell only if a mpcekf_set_limits is still in force.
 * mpcekf_thermal_end does the same implicitly.  A no-op without a schedule. */
int mpcekf_thermal_schedule_end(mpcekf_ctx *ctx);

/* ---- the MPC limits mapped over the SOC estimate and the temperature (not part of the reference interface) ----
 * The charger a fast-charge controller is compared against is a current map over state of charge
 * and temperature: multi-stage constant current, a C-rate that steps down at 40 / 60 / 80 % SOC,
 * then constant voltage.  A limit map is sets of 2-D tables of limit fields over (SOC estimate,
 * cell temperature) on uniform grids, evaluated per cell on the device in every fused step -- on
 * every fused route: mpcekf_step, every _step_ex_*, mpcekf_step_summary, mpcekf_step_until and
 * graph replay; with packs, the balancer, the charger, termination, the aging record and the
 * thermal model with links.  Like the temperature schedule it writes rows of the per-cell limits
 * record and changes no QP structure.
 *
 * fields[nfields]: distinct ids among MPCEKF_LIM_CRATE, _U_MAX, _DU_MIN, _DU_MAX, _V_MAX,
 * _PHISE_MIN.  tables [nsets][nfields][nt][nz] in mpcekf_config's units: entry [jt][jz] of a table
 * is the field's value at SOC z_lo + jz (z_hi - z_lo) / (nz - 1) (a fraction, as mpcekf_traj.soc)
 * and T_lo + jt (T_hi - T_lo) / (nt - 1) degC.  nz >= 1, nt >= 1, not both 1.  nt >= 2 needs a
 * thermal model (MPCEKF_E_STATE without one); nt == 1 ignores the temperature (T_lo_degC and
 * T_hi_degC are not read) and works on any context.  interp_z: 0 linear in SOC; 1 hold, the left
 * node's value, so a staircase is exact without steep ramps (node jz then holds on
 * [z_jz, z_jz+1), node nz - 2 up to z_hi and beyond: the last column is never the value).  The
 * temperature axis is always linear.  set_of_cell [ncells]: each cell's table set 0..nsets-1;
 * NULL: set 0.  z0 [ncells]: the SOC fraction to evaluate at until a fused step has produced an
 * estimate, finite or NaN; NULL: the record's Z_LAST as it stands when the call replaces an
 * active map, NaN otherwise -- for a first map and for one set after mpcekf_limit_map_end alike
 * (no step stores Z_LAST while no map is active, so a caller that resumes passes the soc row it
 * last read).
 *
 * The rule.  For fused step t and each mapped field, the MPC stage of step t reads the table
 * value at
 *   z: the soc row (zk(end), mpcekf_traj.soc) of the previous fused step, kept per cell in the
 *      record's Z_LAST row.  Every fused step stores it (a cell in error stores NaN); neither
 *      mpcekf_init_cells nor mpcekf_set_state touches it.  The estimate of step t itself is formed
 *      inside the kernel whose MPC stage reads the limits, so the one-step lag is part of the rule;
 *   T: the temperature step t uses (temp[t] of mpcekf_step_ex_thermal).
 * Per cell, every line one or more separately rounded fp64 operations in exactly this order (no
 * contraction, IEEE division):
 *   xz = (z - z_lo) / (z_hi - z_lo);  xzc = xz > 0 ? xz : 0;  xzc = xzc < 1 ? xzc : 1   (NaN -> 0)
 *   sz = xzc * (double)(nz - 1);  jz = min((int)sz, nz - 2);  fz = interp_z ? 0.0 : sz - (double)jz
 *             (nz == 1: jz = 0, and no second column is read)
 *   xt, st, jt, ft likewise over T, T_lo, T_hi, nt    (nt == 1: jt = 0, and no second row is read)
 *   a   = tab[jt][jz]   + fz * (tab[jt][jz+1]   - tab[jt][jz])          (nz == 1: a = tab[jt][0])
 *   b   = tab[jt+1][jz] + fz * (tab[jt+1][jz+1] - tab[jt+1][jz])        (nt >= 2 only)
 *   val = a + ft * (b - a)                                              (nt == 1: val = a)
 * The kernels' slot is formed from val by the expression the scalar configuration goes through
 * (u_min = -Q * val for CRATE, val itself for the others).  So with nz == 1 the map is
 * mpcekf_thermal_schedule's lookup bit for bit, and a table constant at the configuration's value
 * feeds the MPC kernels the scalar's bits.
 *
 * A fused call evaluates once before its first step, at Z_LAST and the temperature as they stand,
 * and at the end of every step that another step of the call follows; the call's last step stores
 * Z_LAST (and advances the model) but evaluates nothing, so the values in force after a call are
 * what its last step used.  N one-step calls and one N-step call compute the same.
 *
 * The record, per cell, every value a double and the counts exact integers: */
enum {
  MPCEKF_LM_Z_LAST = 0, /* the soc row of the last fused step (z0 until there is one) */
  MPCEKF_LM_NEVAL,      /* evaluations made for fused steps since the map was set: one per step */
  MPCEKF_LM_NCLAMP_Z,   /* those whose xz fell outside [0, 1] or was NaN */
  MPCEKF_LM_NCLAMP_T,   /* the same for xt (stays 0 with nt == 1) */
  MPCEKF_NLM
};
/* Setting a map moves the context to the per-cell launch sequence if it is not
 * there already, restarts the record's counts and evaluates once at Z_LAST and the temperatures as
 * they stand (this evaluation, and the one a mpcekf_set_limits of another field repeats, are not
 * counted in the record).  A second call replaces the map (fields of the first that the second
 * does not name go back to their mpcekf_set_limits / configuration values); captured graphs stay
 * valid.  The map and a temperature schedule exclude each other: whichever is set second returns
 * MPCEKF_E_STATE and changes nothing.  While a map is active, mpcekf_get_limits returns for a
 * mapped field the value in force after the last evaluation; mpcekf_set_limits naming a mapped
 * field returns MPCEKF_E_ARG and mpcekf_clear_limits returns MPCEKF_E_STATE, both changing
 * nothing.  mpcekf_thermal_end ends a map that has nt >= 2.  The stage route does not evaluate the
 * map: it reads the values of the last evaluation.  The map's kernels are not among
 * mpcekf_set_timing's five slots.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx, fields or tables; nfields outside 1..6; a repeated
 * id or one that cannot be mapped; nz < 1, nt < 1 or both 1; z_lo or z_hi not finite, or
 * z_hi <= z_lo; with nt >= 2, T_lo or T_hi not finite, or T_hi <= T_lo; interp_z outside {0, 1};
 * nsets < 1; a non-finite table entry; a set_of_cell entry outside 0..nsets-1; an infinite z0
 * entry (the message names the cell). */
int mpcekf_limit_map(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, int32_t nz, double z_lo, double z_hi,
                     int32_t nt, double T_lo_degC, double T_hi_degC, int32_t interp_z, int32_t nsets,
                     const double *tables, const int32_t *set_of_cell, const double *z0);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_LM_* ids).  MPCEKF_E_STATE
 * without a map; MPCEKF_E_ARG: a NULL pointer, nfields outside 1..MPCEKF_NLM, an unknown or
 * repeated id. */
int mpcekf_limit_map_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Ends the map: its fields go back to what mpcekf_set_limits or the configuration last gave them,
 * and the launch sequence stays per-cell only if a mpcekf_set_limits is still in force.  The
 * graphs captured with the map are retired.  A no-op without a map. */
int mpcekf_limit_map_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_charger's arguments (each extension's rows must be NULL without that extension
 * -- MPCEKF_E_STATE -- and no charger is needed) plus lim [nsteps][nfields][ncells] (host, or
 * device when outputs_on_device != 0; may be NULL): lim[t][i] is the value of the map's field
 * fields[i] that the MPC stage of step t read, in mpcekf_config's units.  MPCEKF_E_STATE without
 * a map. */
int mpcekf_step_ex_map(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                       const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                       int32_t *limiter, double *bleed, double *zmin, double *vstr, double *istr, int32_t *capby,
                       double *lim, int32_t outputs_on_device);

/* ---- series strings: one current per pack string along the fused loop (not part of the reference interface) ----
 * Cells in series carry one current, and a charger can only apply what the weakest cell of the
 * string accepts.  With a pack, the cells' controllers stay their own and the library couples
 * their commands on the device, once per fused step, after the QP has produced them:
 * - A context with a pack has ncells = nstrings * S.  String g is the cells [g*S, (g+1)*S).
 * - After fused step t has produced each cell's command u_c, the kernel picks one cell per
 *   string, the limiter.
 *   - u_c is what Hildreth, or the unconstrained path, stored into s.uk (MPCEKF_S_UK).  Charging
 *     current is negative, initMPC.m:66-67.
 *   - The limiter is the cell with the largest u_c among the cells whose u_c is not NaN.
 *   - Comparison is by value, so -0.0 == +0.0.  Ties go to the lowest in-string index.
 * - The string current m_g is the limiter's u_c, bit for bit.  Every cell of the string whose own
 *   command is not NaN gets s.uk <- m_g and s.uk_1 <- m_g (MPCEKF_S_UK, MPCEKF_S_UK_1).
 * - A cell whose command is NaN (error, lock-out) is excluded.  It keeps its NaN, and its s.uk_1
 *   is not touched.
 * - A string with no non-NaN command writes nothing.  Its limiter is -1.
 * - The u row of the step (trajectory, device buffer, summary window) holds the applied current
 *   m_g for the cells that received it.  Excluded cells keep their NaN.
 * - Because u holds the applied current, three things see it without further change:
 *   - k_summary's peak current and charge moved (mpcekf_step_summary);
 *   - the thermal model's carried current, which k_thermal reads from s.uk after this kernel;
 *   - the next step's uk_1, and the uk_1 copy that k_cl_diag uses (poles / sv).
 * - Per-cell record, [ncells] each, accumulated over any number of calls and reset by begin,
 *   every value a double, counts exact integers:
 *   - NLIM: the number of steps this cell was its string's limiter.
 *   - STEPS: the number of steps this cell had a non-NaN command.
 *   - HEADROOM: the sequential sum in step order of m_g - u_c, one rounded subtraction and one
 *     rounded addition per step, from +0.  Only finite terms are added.  The unit is A*steps: the
 *     charging current the cell would have taken but did not.
 * - S = 1 is the identity.  Such a context runs the same bits as one without a pack (the record
 *   still counts: NLIM = STEPS, HEADROOM sums zeros).
 * The pack is a property of the context, like the thermal model: mpcekf_step, _step_ex,
 * _step_ex_obs, _step_ex_thermal, _step_summary and _step_ex_pack all run the pack step, graph
 * replay included.  The stage route (mpcekf_mpc_step(_ex)) is not coupled: a host loop over the
 * stage calls sees every cell's own command, as it does not advance the thermal model either.
 * The pack's kernel is not one of mpcekf_set_timing's five slots.
 * Heat conduction between neighbouring cells of a string: mpcekf_thermal_couple, below.
 * Passive balancing (a bleed current around the cells that are ahead): mpcekf_balance_begin, below.
 * Not modelled: parallel groups, active balancing, strings of unequal length. */
enum { MPCEKF_PK_NLIM = 0, MPCEKF_PK_STEPS, MPCEKF_PK_HEADROOM, MPCEKF_NPK };
/* Makes the context a pack of ncells / series strings of `series` cells each, allocates the
 * record (first call) and resets it; a second begin replaces the first and resets the record.
 * May be called before mpcekf_init_cells.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx, series < 1, ncells % series != 0. */
int mpcekf_pack_begin(mpcekf_ctx *ctx, int32_t series);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_PK_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NPK, an unknown or repeated id. */
int mpcekf_pack_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the record; the cells keep their state and the context then behaves as one that never
 * began.  A no-op without a begin. */
int mpcekf_pack_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_obs (and, on a thermal context, mpcekf_step_ex_thermal: temp / heat, which
 * must be NULL without a model -- MPCEKF_E_STATE -- as tc_degC must be NULL with one) on a
 * pack context plus the pack's rows (host, or device when outputs_on_device != 0), either may
 * be NULL: ucmd [nsteps][ncells], each cell's own command before the reduction (traj->u holds
 * the applied current); limiter [nsteps][ncells / series], each string's limiter as an
 * in-string index, or -1.  MPCEKF_E_STATE without a begin; a refused call leaves the context
 * and the record as they were. */
int mpcekf_step_ex_pack(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                        const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                        int32_t *limiter, int32_t outputs_on_device);

/* ---- passive balancing of pack strings: bleed currents along the fused loop (not part of the reference interface) ----
 * A string that starts with an SOC spread keeps it: every cell gets the same current, the cell
 * that is furthest ahead becomes the limiter and the others stop short of the target.  A passive
 * balancer is a bleed resistor per cell that diverts part of the string current around a cell
 * that is ahead.  A balancer is a property of a pack context (mpcekf_pack_begin first); on such
 * a context the rule below runs once per fused step in k_pack's place, after k_term.
 * Parameters, [ncells] each:
 *   i_bleed    A, >= 0; 0: the cell has no bleeder
 *   dz_on      a SOC fraction in mpcekf_traj.soc's unit, > 0
 *   dz_off     a SOC fraction, 0 <= dz_off <= dz_on (hysteresis)
 *   compensate 0 or 1, one per context
 * Per-cell state: one flag `on`.  It starts at 0, is reset by begin and persists across calls.
 * Inputs at fused step t, for string g = cells [g*S, (g+1)*S), read after k_term:
 *   u_c = the cell's own command in s.uk (MPCEKF_S_UK); for a latched cell the +0.0 k_term wrote
 *   z_c = this step's soc row, zk(end) (mpcekf_traj.soc)
 * 1. A cell is valid when neither u_c nor z_c is NaN.  zmin_g is the smallest z_c over the valid
 *    cells of the string.  Comparison is by value; on a tie the lowest in-string index wins, and
 *    zmin_g is that cell's z_c bit for bit.  If the string has no valid cell, zmin_g is NaN.
 * 2. For a valid cell, d = z_c - zmin_g, one rounded subtraction.
 *      if d >= dz_on:        on = 1
 *      else if d <= dz_off:  on = 0
 *      else:                 on keeps its value
 *    For a cell that is not valid, on = 0.
 *    The cell is bleeding when on && i_bleed_c > 0.  b_c = i_bleed_c when bleeding, else +0.0.
 * 3. The effective command is e_c = u_c - b_c (one rounded subtraction) when
 *    compensate && bleeding && u_c < 0.  Otherwise e_c = u_c bit for bit.  So with compensate on,
 *    the charger supplies what the cell accepts plus what its bleeder diverts.  A resting or
 *    latched cell has u_c = +0.0, which is not < 0, so it is never compensated and still stops
 *    its string.
 * 4. The limiter is chosen by the pack's rule applied to e_c: the largest e_c among the cells
 *    whose u_c is not NaN, compared by value, on a tie the lowest in-string index wins.
 *    m_g = e_lim, bit for bit.  A string with no non-NaN command writes nothing to s.uk, s.uk_1
 *    and the u row, and its limiter is -1.
 * 5. The applied current is a_c = m_g + b_c (one rounded addition) for a bleeding cell.  For any
 *    other cell with a non-NaN command it is a_c = m_g, bit for bit.  s.uk, s.uk_1 and the
 *    step's u row get a_c.  A cell with a NaN command keeps its NaN, and its s.uk_1 is
 *    untouched.  Everything downstream reads these locations, so it sees the cell's own current
 *    with no further change: the plant, the EKF's ik, the summary's current and charge, k_aging
 *    and k_thermal's carried current.
 * 6. Records.  The pack record keeps its three fields, with e_c in u_c's place: STEPS += 1 for
 *    a non-NaN command, NLIM += 1 for the limiter on e, HEADROOM += m_g - e_c (finite terms
 *    only).  The balance record, [ncells] each, every value a double, counts exact integers,
 *    accumulated over any number of calls and reset by begin:
 *      STEPS_ON   the steps the cell was bleeding
 *      Q_BLEED    the sequential sum in step order of b_c over the bleeding steps, from +0, A*steps
 *      SWITCHES   the off -> on transitions of `on`
 *      DZ_MAX     the largest non-NaN d seen; NaN: none
 *      DZ_LAST    d of the latest step; NaN for a cell that is not valid
 *      STEPS      the steps the cell was valid
 * Identities: i_bleed = 0 everywhere leaves every bit of the same pack context without a
 * balancer.  A dz_on that no cell reaches leaves every bit too.  S = 1 is the identity, because
 * d = 0 < dz_on.
 * The balancer is a property of the context, like the pack: mpcekf_step, _step_ex, _step_ex_obs,
 * _step_ex_thermal, _step_ex_pack, _step_ex_aging, _step_ex_couple, _step_ex_balance,
 * _step_summary and _step_until all run it, graph replay included, at every horizon and on every
 * route of the fused step, in the same launch that couples the strings.  mpcekf_get_state /
 * mpcekf_set_state do not carry the flag.  The kernel is not one of mpcekf_set_timing's five
 * slots.
 * Not modelled: a voltage-based criterion, a bleed current that depends on the cell voltage
 * (v / R), the bleeder's own heat in the thermal model, active (charge-shuttling) balancing, the
 * stage route (mpcekf_mpc_step(_ex) neither couples nor balances). */
enum { MPCEKF_BLP_I_BLEED = 0, MPCEKF_BLP_DZ_ON, MPCEKF_BLP_DZ_OFF, MPCEKF_NBLP };
enum {
  MPCEKF_BL_STEPS_ON = 0, MPCEKF_BL_Q_BLEED, MPCEKF_BL_SWITCHES, MPCEKF_BL_DZ_MAX, MPCEKF_BL_DZ_LAST,
  MPCEKF_BL_STEPS, MPCEKF_NBL
};
/* Gives the pack context a balancer: params [MPCEKF_NBLP][ncells], compensate 0 or 1.  Allocates
 * the balancer's device buffers (first call) and resets the flags and the record; a second begin
 * replaces the first and resets likewise.  May be called before mpcekf_init_cells.  A later
 * mpcekf_pack_begin with another series keeps the balancer (parameters and flags are per cell);
 * mpcekf_pack_end ends it.
 * MPCEKF_E_STATE (nothing changed): no pack.  MPCEKF_E_ARG (nothing changed): a NULL pointer, a
 * negative or NaN i_bleed, dz_on <= 0 or NaN, dz_off outside [0, dz_on], a compensate that is
 * not 0 / 1. */
int mpcekf_balance_begin(mpcekf_ctx *ctx, const double *params, int32_t compensate);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_BL_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NBL, an unknown or repeated id. */
int mpcekf_balance_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the balancer; the cells keep their state and the context then behaves as a pack that
 * never had one.  A no-op without a begin. */
int mpcekf_balance_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_pack's arguments plus the balancer's rows (host, or device when
 * outputs_on_device != 0), either may be NULL: bleed [nsteps][ncells], b_c, NaN for a cell with
 * a NaN command; zmin [nsteps][ncells / series], zmin_g.  MPCEKF_E_STATE without a balancer; a
 * refused call leaves the context and the records as they were. */
int mpcekf_step_ex_balance(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                           const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                           int32_t *limiter, double *bleed, double *zmin, int32_t outputs_on_device);

/* ---- charger limits on pack strings: string voltage, current and power caps (not part of the reference interface) ----
 * A string's current is bounded by its cells; a real charger adds a current and a power rating
 * of its own.  At low SOC a long string asks for more power than any charger delivers, and the
 * power-limited phase is the interesting part of a fast charge.  A charger is a property of a
 * pack context (mpcekf_pack_begin first; a balancer may or may not be present).  On such a
 * context the rule below runs once per fused step, after k_term, in the launch that couples the
 * strings (k_charger in k_pack's or k_pack_bal's place): the charger adds no launch.
 * Parameters, [nstrings] each (nstrings = ncells / series):
 *   i_max   A, >= 0, or NaN: no current cap.  +inf is allowed and never binds.
 *   p_max   W, > 0, or NaN: no power cap.  +inf is allowed and never binds.
 * At fused step t, for string g = cells [g*S, (g+1)*S):
 * 1. Terms.  v_i is the cell's s.vk (MPCEKF_S_VK), the plant voltage this step measured.  When
 *    the cell's command in s.uk and v_i are both not NaN, x_i = v_i + 0.0 (one rounded addition,
 *    which turns a -0.0 into +0.0) and the cell contributed.  Otherwise x_i = +0.0.  nvalid_g
 *    counts the cells that contributed.
 * 2. String voltage, a fixed tree over the in-string index i = 0 .. S-1:
 *      for level j = 0, 1, ... while 2^j < S:
 *        for every i that is a multiple of 2^(j+1) with i + 2^j < S:
 *          x_i <- x_i + x_(i + 2^j)          (one rounded addition)
 *      V_g = x_0
 *    A partner at or beyond S is skipped.  No term is -0.0, so no partial sum is, and skipping
 *    equals adding +0.0.  The shape depends on S only, never on the block, the wave or the lane a
 *    cell sits in.  A floating-point sum is not associative: another order gives other bits.
 * 3. String current before the charger.  m_g and the limiter come from the pack's rule, or, with
 *    a balancer, from steps 1 to 4 of the balance rule (m_g = e_lim).  A string with no non-NaN
 *    command writes nothing to s.uk, s.uk_1 and the u row: limiter = -1, capby = -1, istr = NaN,
 *    and the charger record counts nothing.  vstr is still V_g.
 * 4. Caps.  Charging current is negative, so a cap is a lower bound.
 *      cap_i = -i_max                when i_max is not NaN
 *      cap_p = -(p_max / V_g)        when p_max is not NaN and V_g > 0 (one rounded division, an
 *                                    exact negation)
 *    cap is the larger of the two by value; on a tie the current cap wins.  If a cap exists and
 *    cap > m_g by value, then m'_g = cap bit for bit, capby = 1 (current) or 2 (power), and the
 *    step's limiter entry is -2: no cell set the current.  Otherwise m'_g = m_g bit for bit,
 *    capby = 0 and the limiter is unchanged.  A resting string (m_g = +0.0) and a discharging one
 *    are never capped.
 * 5. Applied current: the pack's rule, or step 5 of the balance rule, with m'_g in m_g's place.
 *    a_c = m'_g + b_c (one rounded addition) for a bleeding cell, else a_c = m'_g.  s.uk, s.uk_1
 *    and the step's u row get a_c; a cell with a NaN command is untouched.  The plant, k_summary,
 *    k_aging, k_thermal, the next step's uk_1 and k_cl_diag read these locations, so they see
 *    the capped current with no change of their own.
 * 6. Records.  The pack record keeps its fields with m'_g in m_g's place: HEADROOM += m'_g - e_c
 *    (e_c = u_c without a balancer), and NLIM counts nothing on a capped step.  The balance record
 *    is unchanged.  The charger record, [nstrings] each, every value a double, counts exact
 *    integers, sums sequential in step order from +0 with only finite terms added, accumulated
 *    over any number of calls and reset by begin; a step counts when the string has a current:
 *      STEPS       the steps with a string current
 *      NCAP_I      the steps the current cap set the current
 *      NCAP_P      the steps the power cap set the current
 *      Q           the sum of m'_g, A*steps
 *      E           the sum of V_g * m'_g (one rounded product), W*steps: the charger's own
 *                  estimate, from the voltage measured under the previous step's current
 *      CURTAIL     the sum of m'_g - m_g (one rounded subtraction), A*steps
 *      P_MIN       the smallest product V_g * m'_g seen (the largest charging power); NaN: none
 *      V_PEAK      the largest V_g seen; NaN: none
 *      NVALID_MIN  the smallest nvalid_g seen; NaN: none
 * 7. Identities.  Both parameters NaN (or +inf) everywhere leaves every bit of the same pack or
 *    balancer context without a charger: u, ucmd, limiter, bleed, zmin, both older records and
 *    the final state.  S = 1 works, with V_g = v + 0.0.
 * The charger is a property of the context, like the pack: mpcekf_step, every _step_ex_*,
 * _step_summary and _step_until run it, graph replay included, at both horizons and on every
 * route of the fused step.  The kernel is not one of mpcekf_set_timing's five slots.
 * Not modelled: a pack voltage limit or CV loop, charger efficiency, the stage route
 * (mpcekf_mpc_step(_ex) neither couples nor caps), mpcekf_get_state / mpcekf_set_state carrying
 * the record. */
enum { MPCEKF_CHP_I_MAX = 0, MPCEKF_CHP_P_MAX, MPCEKF_NCHP };
enum {
  MPCEKF_CH_STEPS = 0, MPCEKF_CH_NCAP_I, MPCEKF_CH_NCAP_P, MPCEKF_CH_Q, MPCEKF_CH_E, MPCEKF_CH_CURTAIL,
  MPCEKF_CH_P_MIN, MPCEKF_CH_V_PEAK, MPCEKF_CH_NVALID_MIN, MPCEKF_NCH
};
/* Gives the pack context a charger: params [MPCEKF_NCHP][nstrings].  Allocates the charger's
 * device buffers (first call) and resets the record; a second begin replaces the first and
 * resets likewise.  May be called before mpcekf_init_cells.  A later mpcekf_pack_begin with
 * another series ends the charger (its arrays are per string); mpcekf_pack_end ends it.
 * MPCEKF_E_STATE (nothing changed): no pack.  MPCEKF_E_ARG (nothing changed): a NULL pointer, a
 * negative i_max, p_max <= 0. */
int mpcekf_charger_begin(mpcekf_ctx *ctx, const double *params);
/* values [nfields][nstrings]: row i = field fields[i] (distinct MPCEKF_CH_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NCH, an unknown or repeated id. */
int mpcekf_charger_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the charger; the cells keep their state and the context then behaves as a pack that
 * never had one.  A no-op without a begin. */
int mpcekf_charger_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_balance's arguments (bleed / zmin must be NULL without a balancer --
 * MPCEKF_E_STATE) plus the charger's rows (host, or device when outputs_on_device != 0), each
 * may be NULL, [nsteps][ncells / series] each: vstr, V_g; istr, m'_g (NaN for a string without
 * a current); capby, int32: -1 / 0 / 1 / 2.  MPCEKF_E_STATE without a charger; a refused call
 * leaves the context and the records as they were. */
int mpcekf_step_ex_charger(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                           const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                           int32_t *limiter, double *bleed, double *zmin, double *vstr, double *istr, int32_t *capby,
                           int32_t outputs_on_device);

/* ---- side-reaction losses per cell along the fused loop (not part of the reference interface) ----
 * runMPC.m keeps phise_store above mpcData.const.phise_min so that lithium does not plate.  How
 * much a protocol plated, or how much SEI (the solid-electrolyte interphase film on the negative
 * electrode) it grew, is the integral over the charge of a Tafel-type side-reaction current
 * driven by the side-reaction overpotential and the temperature.  A context can carry up to four
 * such reactions per cell, each evaluated from the EKF's estimate (source EST), from the plant's
 * own value (source PLANT), or both: what the controller believed it plated beside what the
 * plant plated.
 * Per cell c, after fused step t, for every enabled source s and every reaction r, every line
 * one or more separately rounded fp64 operations in exactly this order (no contraction into
 * fused multiply-adds, IEEE division, dexp the defined exp of the v3 Arrhenius factor: rom.py
 * dexp, oracle/mpcekf_oracle.c orc_exp); F, R and Tref are the ROM's (mpcekf_rom):
 *   T    = the temperature step t used: temp[t] of mpcekf_step_ex_thermal (the cell temperature
 *          after the step has stored its tc_degC row, before the thermal model advances it)
 *   TK   = T + 273.15
 *   phi  = source EST:   phise_store(t), the step's traj.phise row (runMPC.m:94-95)
 *          source PLANT: the negPhise0 slot of step t's row of mpcekf_step_ex_obs
 *   eta  = phi - U_r
 *   g    = (alpha_r * F) / (R * TK)
 *   ar   = dexp((Ea_r / R) * (1.0 / Tref - 1.0 / TK))
 *   j    = (i0_r * ar) * dexp(-(g * eta))           amperes; Tafel, cathodic
 *   on   = eta < gate_r                             false for a NaN eta; gate = +inf: always on
 *   if on and isfinite(j):
 *          Q_SUM <- Q_SUM + j                       plain additions from +0 in step order
 *                                                   (Ah = Q_SUM * Ts / 3600)
 *          N_ON  <- N_ON + 1
 *          if isnan(J_MAX) or j > J_MAX:            strict comparison: the first occurrence wins
 *                 J_MAX <- j;  J_MAX_STEP <- tt
 *   per source: STEPS += 1 if phi is not NaN, else NSKIP += 1
 *   tt = STEPS + NSKIP + 1, read from the record before the update
 * tt counts the source's steps since begin, from 1, across calls.  A cell in error or lock-out
 * has a NaN phise from its failing step on: NSKIP counts those steps and the sums stay.
 * The record, every value a double, counts and step indices exact integers: Q_SUM, J_MAX (NaN
 * before the first step taken), J_MAX_STEP (0 likewise), N_ON per source and reaction; STEPS and
 * NSKIP per source, the same for every reaction.
 * The aging record is a property of the context, like the thermal model: mpcekf_step, _step_ex,
 * _step_ex_obs, _step_ex_thermal, _step_ex_pack, _step_summary and _step_ex_aging all
 * accumulate, graph replay included.  The stage route does not accumulate, as it does not
 * advance the thermal model.  mpcekf_get_state / mpcekf_set_state carry neither the aging record
 * nor the thermal one.  The kernel is not one of mpcekf_set_timing's five slots.
 * Not modelled: stripping of plated lithium, feedback of the lost capacity into the plant. */
#define MPCEKF_AG_SRC_EST 1   /* the EKF's estimate, phise_store                         */
#define MPCEKF_AG_SRC_PLANT 2 /* the plant's own negPhise0 (OB_step.m:317)               */
#define MPCEKF_AG_MAXREACT 4
enum {
  MPCEKF_AG_I0 = 0 /* A, at Tref and eta = 0 */, MPCEKF_AG_U /* V */, MPCEKF_AG_ALPHA, MPCEKF_AG_EA /* J/mol */,
  MPCEKF_AG_GATE /* V, +inf: always on */, MPCEKF_NAGP
};
enum {
  MPCEKF_AGR_Q_SUM = 0, MPCEKF_AGR_J_MAX, MPCEKF_AGR_J_MAX_STEP, MPCEKF_AGR_N_ON, MPCEKF_AGR_STEPS,
  MPCEKF_AGR_NSKIP, MPCEKF_NAGR
};
/* Gives the context nreact reactions evaluated from the sources of the bit mask `sources`
 * (MPCEKF_AG_SRC_*): params [nreact][MPCEKF_NAGP][ncells].  Allocates the record (first call) and
 * resets it; a second begin replaces the first.  May be called before mpcekf_init_cells.
 * MPCEKF_E_ARG (nothing changed): a NULL pointer; nreact outside 1..4; sources outside 1..3; an
 * i0 that is not finite or is negative; a non-finite U or Ea; an alpha that is not finite and
 * positive; a NaN gate.  MPCEKF_E_UNSUPPORTED: source PLANT on a ROM whose obs layout has no
 * negPhise0 (none today: mpcekf_ctx_create refuses a ROM without exactly one phise row at the
 * negative collector with MPCEKF_E_ROM). */
int mpcekf_aging_begin(mpcekf_ctx *ctx, int32_t nreact, int32_t sources, const double *params);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_AGR_* ids) of source
 * `source` (one MPCEKF_AG_SRC_* bit the begin enabled), reaction `react` (0..nreact-1).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, a source that is not enabled, a
 * react outside 0..nreact-1, nfields outside 1..MPCEKF_NAGR, an unknown or repeated id. */
int mpcekf_aging_get(mpcekf_ctx *ctx, int32_t source, int32_t react, int32_t nfields, const int32_t *fields,
                     double *values);
/* Frees the record; the context then behaves as one that never began.  A no-op without a begin. */
int mpcekf_aging_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_pack's arguments (ucmd / limiter need a pack, temp / heat a model:
 * MPCEKF_E_STATE without) plus rate [nsteps][nsrc * nreact][ncells] (host, or device when
 * outputs_on_device != 0; may be NULL): the enabled sources in id order, the reactions inside.
 * A rate row holds j where on && isfinite(j), NaN where phi is NaN, +0.0 otherwise.
 * MPCEKF_E_STATE without a begin; a refused call leaves the context and the record as they were. */
int mpcekf_step_ex_aging(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                         const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                         int32_t *limiter, double *rate, int32_t outputs_on_device);

/* ---- heat conduction between neighbouring cells of a pack string (not part of the reference interface) ----
 * The thermal model above exchanges heat with each cell's own ambient only, so a string of
 * identical cells stays identical.  In a module the inner cells run hotter than the end cells.
 * A context that has both a thermal model (mpcekf_thermal_begin) and a pack (mpcekf_pack_begin)
 * can be given links: r_link[c] is the thermal resistance in K/W between cell c and cell c+1.
 * It is used only when both cells are in the same string; the entry of a string's last cell is
 * ignored; +inf means no link.
 * Per cell c at in-string position p = c mod S, after fused step t: T, q and loss are exactly
 * as in the thermal model's recurrence.  Tl and Tr are the temperatures that step t used for
 * the cells c-1 and c+1: their temp[t], not values already advanced in this launch.  Every line
 * one or more separately rounded fp64 operations in exactly this order (no contraction into
 * fused multiply-adds, IEEE division):
 *   qn = +0.0;  nl = 0
 *   if p > 0     and isfinite(r_link[c-1]):  dl = Tl - T;  qn = qn + dl / r_link[c-1];  nl += 1
 *   if p < S - 1 and isfinite(r_link[c]):    dr = Tr - T;  qn = qn + dr / r_link[c];    nl += 1
 *   Tn = nl == 0 ? T + ((q - loss) * Ts) / Cth              the uncoupled line, bit for bit
 *                : T + (((q - loss) + qn) * Ts) / Cth
 *   T <- Tn if isfinite(Tn) and Tn <= 100; otherwise T is held: the accept-or-hold rule is unchanged
 * A cell whose T is held because it is in error (its q is NaN) keeps its finite T, and its
 * neighbours still conduct to and from it.  Tl - T on one side of a link and T - Tr on the other
 * are exact negatives (an fp64 subtraction with its operands swapped gives the negated result),
 * and both are divided by the same r_link: the two flows over a link cancel exactly, so
 * conduction moves heat and makes none.
 * The record, per cell, every value a double, step indices exact integers that count the
 * model's steps from 1 across calls, as T_MAX_STEP does:
 *   NB_SUM       qn added in step order, plain fp64 additions from +0: only finite values, and
 *                only on steps with nl > 0 (energy in J = NB_SUM * Ts)
 *   DT_MAX, DT_MAX_STEP   the largest |dl| or |dr| over the cell's finite links and the step it
 *                occurred in; within a step the left link is examined first; replaced only on a
 *                strict >.  NaN / 0 before the first such step
 * The links are a property of the context: once set, mpcekf_step, _step_ex, _step_ex_obs,
 * _step_ex_thermal, _step_ex_pack, _step_ex_aging, _step_summary and _step_ex_couple all run
 * the coupled step, graph replay included.  The stage route does not advance the model, as
 * ever.  S = 1, or every link +inf, runs the uncoupled model's bits.  The kernels are not among
 * mpcekf_set_timing's five slots.
 * Not modelled: 2-D or 3-D neighbourhoods, conduction between strings, tab or busbar heat. */
enum { MPCEKF_TCR_NB_SUM = 0, MPCEKF_TCR_DT_MAX, MPCEKF_TCR_DT_MAX_STEP, MPCEKF_NTCR };
/* Sets the links: r_link [ncells].  Allocates the coupling's device buffers (first call) and
 * resets the record; a second call replaces the links and resets the record.  Every entry is
 * validated, the ignored string-end entries included, so a later mpcekf_pack_begin with another
 * series is safe: a second mpcekf_pack_begin keeps the coupling, the links following the new
 * strings; a second mpcekf_thermal_begin keeps it and resets its record.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx or r_link; an entry that is NaN or not > 0 (+inf
 * allowed).  MPCEKF_E_STATE (nothing changed): no thermal model, or no pack. */
int mpcekf_thermal_couple(mpcekf_ctx *ctx, const double *r_link);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_TCR_* ids).
 * MPCEKF_E_STATE without links; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NTCR, an unknown or repeated id. */
int mpcekf_thermal_couple_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* Frees the links and the record; the context then runs the uncoupled model again.
 * mpcekf_thermal_end and mpcekf_pack_end do the same implicitly.  A no-op without links. */
int mpcekf_thermal_couple_end(mpcekf_ctx *ctx);
/* mpcekf_step_ex_aging's arguments (rate needs an aging record: MPCEKF_E_STATE without) plus
 * cond [nsteps][ncells] (host, or device when outputs_on_device != 0; may be NULL): each step's
 * qn, +0.0 where nl == 0.  MPCEKF_E_STATE without links; a refused call leaves the context and
 * the records as they were. */
int mpcekf_step_ex_couple(mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj,
                          const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                          int32_t *limiter, double *rate, double *cond, int32_t outputs_on_device);

/* ---- charge termination along the fused loop (not part of the reference interface) ----
 * runMPC.m steps its one cell for a fixed time, and its z_max row holds the SOC at the target for
 * the rest of it.  A charger terminates: at a SOC, in the CV phase once the current has tapered
 * below a threshold for a few samples, or on a temperature cut-off.  With a termination rule the
 * context decides per cell, on the device, once per fused step, after the QP has produced the
 * cell's command, whether the cell is done; a done cell rests at 0 A from then on, and
 * mpcekf_step_until stops the loop when no cell is left.
 * Parameters, [ncells] each; a NaN turns its criterion off, which falls out of the comparisons:
 *   soc_stop   a fraction 0..1, in mpcekf_traj.soc's unit, like soc_reach
 *   i_taper    A
 *   T_cut      degC
 *   hold       a step count >= 1, one per context
 * Per-cell state: OPEN (initial), LATCHED or DEAD.  t counts the fused steps since
 * mpcekf_term_begin, from 1, across calls.
 * Inputs at step t, read after Hildreth, the slow path and k_cl_diag, and before k_pack:
 *   z = this step's soc row, zk(end) (mpcekf_traj.soc)
 *   u = the cell's own command in s.uk (MPCEKF_S_UK)
 *   T = s.Tc, the temperature the step used, whatever set it (temp[t] of mpcekf_step_ex_thermal)
 * For an OPEN cell, in this order (STEPS += 1 first: for an OPEN cell STEPS == t):
 *   a. If z or u is NaN, the cell becomes DEAD and DONE_STEP = t.  Nothing else changes, now or
 *      later.
 *   b. On a pack (mpcekf_pack_begin, S > 1): if the cell's string had a LATCHED cell after step
 *      t - 1, the cell becomes LATCHED with REASON = 8.  So string-mates follow one step late.
 *      The lag is part of the rule: during the lag step k_pack already gives the string 0 A,
 *      because the latched cell's +0 is the largest command.  The taper counter is not advanced.
 *   c. Otherwise:
 *      if fabs(u) > i_taper:                    armed = 1;  run = 0
 *      else if armed and fabs(u) <= i_taper:    run += 1
 *      else:                                    run = 0
 *      REASON = (z >= soc_stop ? 1 : 0) | (run >= hold ? 2 : 0) | (T >= T_cut ? 4 : 0)
 *      If REASON is non-zero, the cell becomes LATCHED.
 *      armed and run start at 0: a current that never exceeded i_taper does not count as tapered.
 * On latching: DONE_STEP = t, SOC_DONE = z, U_DONE = u, T_DONE = T.
 * A LATCHED cell, one latched in this step included: if its u is not NaN, s.uk, s.uk_1
 * (MPCEKF_S_UK, MPCEKF_S_UK_1) and the step's u row all become +0.0 (a -0.0 command too), and
 * REST += 1.  A NaN command is left alone, as k_pack leaves it.
 * Downstream, all without further change: a latched cell's +0 is the largest command of its
 * string, so k_pack applies 0 A to the whole string; the plant, the EKF's ik, the summary's
 * charge, k_aging and k_thermal all see a resting cell, and k_thermal lets it cool.
 * The record, [ncells] each, every value a double, counts and step indices exact integers:
 *   STATE      MPCEKF_TERM_OPEN, _LATCHED or _DEAD
 *   DONE_STEP  the step the cell latched or died in; 0: none
 *   REASON     the bits above; 0 for an OPEN or DEAD cell
 *   SOC_DONE, U_DONE, T_DONE   z, u and T of the latching step; NaN: none
 *   REST       the steps the cell's command was replaced by +0.0
 *   STEPS      the steps evaluated while OPEN, the latching or dying one included
 * The open counter is one device integer: the number of OPEN cells after the latest step.
 * The rule is a property of the context, like the pack: mpcekf_step, _step_ex, _step_ex_obs,
 * _step_ex_thermal, _step_ex_pack, _step_ex_aging, _step_ex_couple and _step_summary all run it,
 * graph replay included, at every horizon and on every route of the fused step.  The stage route
 * (mpcekf_mpc_step(_ex)) does not run the rule, as it does not couple a pack's strings either.
 * mpcekf_get_state / mpcekf_set_state do not carry the termination state.  A context whose
 * thresholds never hold runs the bits of one without a rule.  The kernel is not one of
 * mpcekf_set_timing's five slots.
 * Not modelled: a T_max row in the QP, resuming a latched cell, skipping a done cell's step. */
enum { MPCEKF_TMP_SOC_STOP = 0, MPCEKF_TMP_I_TAPER, MPCEKF_TMP_T_CUT, MPCEKF_NTMP };
enum { MPCEKF_TERM_OPEN = 0, MPCEKF_TERM_LATCHED, MPCEKF_TERM_DEAD };
enum {
  MPCEKF_TM_STATE = 0, MPCEKF_TM_DONE_STEP, MPCEKF_TM_REASON, MPCEKF_TM_SOC_DONE, MPCEKF_TM_U_DONE,
  MPCEKF_TM_T_DONE, MPCEKF_TM_REST, MPCEKF_TM_STEPS, MPCEKF_NTM
};
/* Gives the context a termination rule: params [MPCEKF_NTMP][ncells], hold >= 1.  Allocates the
 * rule's device buffers (first call) and resets every cell to OPEN, the record, the taper
 * counters and t; a second begin replaces the first and resets likewise.  May be called before
 * mpcekf_init_cells.
 * MPCEKF_E_ARG (nothing changed): a NULL ctx or params, hold < 1. */
int mpcekf_term_begin(mpcekf_ctx *ctx, const double *params, int32_t hold);
/* values [nfields][ncells]: row i = field fields[i] (distinct MPCEKF_TM_* ids).
 * MPCEKF_E_STATE without a begin; MPCEKF_E_ARG: a NULL pointer, nfields outside
 * 1..MPCEKF_NTM, an unknown or repeated id. */
int mpcekf_term_get(mpcekf_ctx *ctx, int32_t nfields, const int32_t *fields, double *values);
/* *open_cells = the open counter (one 4-byte copy).  MPCEKF_E_STATE without a begin;
 * MPCEKF_E_ARG: a NULL pointer. */
int mpcekf_term_open(mpcekf_ctx *ctx, int64_t *open_cells);
/* Frees the rule; the cells keep their state (a latched cell's s.uk is the +0.0 it was given)
 * and the context then behaves as one that never began.  A no-op without a begin. */
int mpcekf_term_end(mpcekf_ctx *ctx);
/* Runs the fused loop with no trajectory output in calls of `chunk` steps (the last one shorter
 * when max_steps % chunk != 0, so a repeated shape replays one graph), reads the open counter
 * after each, and stops when it is 0 or max_steps is reached.  On a context with a summary begun
 * (mpcekf_summary_begin) each chunk is a mpcekf_step_summary call and the record folds as usual;
 * otherwise each chunk is mpcekf_step with NULL outputs.  tc_degC: NULL, or [ncells], the same
 * row for every step; NULL with a thermal model.  *steps_run = the steps run, a multiple of
 * chunk or max_steps; *open_cells = the counter after them (either may be NULL).  By
 * construction the state afterwards is that of plain stepping for *steps_run steps: the
 * overshoot is under `chunk` resting steps.
 * MPCEKF_E_STATE without a mpcekf_term_begin or before mpcekf_init_cells; MPCEKF_E_ARG: a NULL
 * ctx, max_steps < 0, chunk < 1, a tc_degC with a thermal model or out of range.  A refused call
 * changes nothing. */
int mpcekf_step_until(mpcekf_ctx *ctx, int32_t max_steps, int32_t chunk, const double *tc_degC, int32_t *steps_run,
                      int64_t *open_cells);

/* ---- device memory (not part of the reference interface) ----
 * Device buffers for outputs_on_device calls, allocated by the library's own HIP
 * runtime so a host process never holds a second one (a framework's bundled
 * runtime must not hand its pointers to these kernels).  mpcekf_dev_copy is
 * synchronous; kind is MPCEKF_COPY_*.  mpcekf_dev_copy2d copies `height` rows of
 * `width` bytes with the given pitches (e.g. every k-th cell of a [nsteps][ncells]
 * trajectory: width 8, spitch 8k).  mpcekf_sync waits for every launch of the
 * context's device. */
#define MPCEKF_COPY_H2D 0
#define MPCEKF_COPY_D2H 1
#define MPCEKF_COPY_D2D 2
int mpcekf_dev_alloc(int device, int64_t bytes, void **ptr);
int mpcekf_dev_free(void *ptr);
int mpcekf_dev_copy(void *dst, const void *src, int64_t bytes, int32_t kind);
int mpcekf_dev_copy2d(void *dst, int64_t dpitch, const void *src, int64_t spitch, int64_t width, int64_t height,
                      int32_t kind);
int mpcekf_sync(mpcekf_ctx *ctx);  /* also completes the _async stage calls' host outputs */

/* ---- state access (open-loop parity, checkpoint/restore) ---- */
typedef struct {
  double *bigX;    /* [ncells][NM][6]   OB_step cellState.bigX (column per model)     */
  double *ekf;     /* [ncells][NM][20]  per model: xhat[5], SigmaX packed upper [15] */
  double *scal;    /* [ncells][MPCEKF_NSCAL] scalars, see MPCEKF_S_*                 */
  double *lambda;  /* [ncells][ncon]    mpcData.lambda (ncon of mpcekf_ctx_info: enabled rows) */
  int32_t *warn;   /* [ncells]          iterEKF warnCount                            */
  int32_t *status; /* [ncells]          MPCEKF_ST_*                                   */
  double *mb;      /* [ncells][MPCEKF_MB_SIZE] method MB: ekfData.xhat(1:5), 0, SigmaX
                      6x6 row-major (xhat(end) is MPCEKF_S_X0); may be NULL          */
} mpcekf_state;

#define MPCEKF_MB_SIZE 42

#define MPCEKF_S_SOCNAVG 0 /* cellState.SOCnAvg          */
#define MPCEKF_S_SOCPAVG 1 /* cellState.SOCpAvg          */
#define MPCEKF_S_X0 2      /* ekfData.x0                 */
#define MPCEKF_S_SIGMAX0 3 /* ekfData.SigmaX0            */
#define MPCEKF_S_PRIORI 4  /* ekfData.priorI             */
#define MPCEKF_S_UK_1 5    /* mpcData.uk_1               */
#define MPCEKF_S_UK 6      /* command applied next step  */
#define MPCEKF_S_VK 7      /* last plant voltage         */
#define MPCEKF_NSCAL 8

/* Every non-NULL field of st is copied; NULL fields are neither read nor written (a
 * checkpoint without mb restores an MB context's other fields and keeps its blend state). */
int mpcekf_get_state(mpcekf_ctx *ctx, mpcekf_state *st);
int mpcekf_set_state(mpcekf_ctx *ctx, const mpcekf_state *st);
/* The few per-cell scalars a stage-call host reads every step (the MATLAB drop-ins:
 * cellState.SOCnAvg/SOCpAvg before OB_step, OB_step.m:226-228; ekfData.x0, SigmaX0,
 * priorI, warnCount and the status after iterEKF): slots[nslots] are MPCEKF_S_* indices,
 * scal [ncells][nslots]; warn / status [ncells] may be NULL.  Only these bytes cross
 * PCIe: 8 * nslots (+ 4 + 4) per cell. */
int mpcekf_get_scalars(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, double *scal, int32_t *warn,
                       int32_t *status);
int mpcekf_get_scalars_async(mpcekf_ctx *ctx, const int32_t *slots, int32_t nslots, double *scal, int32_t *warn,
                             int32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* MPCEKF_H */
