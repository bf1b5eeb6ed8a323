/*
 * mpcekf_mex.c -- MEX gateway from MATLAB to the MI355X library (include/mpcekf.h).
 *
 * Build (on a machine with MATLAB and the built library; not buildable in this
 * repository's container, which has no MATLAB):
 *   mex -R2018a -I../include mpcekf_mex.c -L../mpc-ekf4fastcharge_amd/_build -lmpcekf
 *
 * One command string per C-ABI entry point, the context kept as a uint64 handle:
 *   h                 = mpcekf_mex('create', R, cfg, device, ncells)   mpcekf_ctx_create
 *                       R: struct from mpcekf_rom_struct(ROM); cfg: struct of mpcekf_config
 *                       fields (missing fields keep the runMPC.m defaults)
 *                       mpcekf_mex('destroy', h)                       mpcekf_ctx_destroy
 *                       mpcekf_mex('init', h, soc0_pct, tc_degC)       mpcekf_init_cells
 *   [u,v,soc,phise,nexec] = mpcekf_mex('step', h, nsteps, tc)          mpcekf_step
 *                       tc: [] or ncells x nsteps (degC); outputs ncells x nsteps
 *   v                 = mpcekf_mex('plant', h, iapp, tc)               mpcekf_plant_step   (OB_step.m:1)
 *   [v,obs]           = mpcekf_mex('plantobs', h, iapp, tc)            mpcekf_plant_step_obs (OB_step.m:1)
 *                       obs: struct with the fields of OB_step's obs (OB_step.m:226-228,289-356),
 *                       each len x ncells (a field without rows in tfData.names is 0 x ncells);
 *                       with one output the record only stays on the device for 'obsslots'
 *   out               = mpcekf_mex('obsslots', h, idx)                 mpcekf_plant_obs_slots
 *                       rows idx (1-based slots of the record, mpcekf_obs_layout) of the last
 *                       'plantobs' record on the device, numel(idx) x ncells
 *   [u,v,soc,phise,nexec,obs] = mpcekf_mex('stepobs', h, nsteps, idx, tc)  mpcekf_step_ex_obs
 *                       'step' plus rows idx (1-based slots of the record) of the plant's
 *                       observables at every step: obs ncells x numel(idx) x nsteps
 *   off               = mpcekf_mex('obslayout', h)                     mpcekf_obs_layout
 *                       1 x 26: field f of obs is slots off(f)+1 .. off(f+1); off(end) = nobs
 *   [zk,zbk,xm,xg]    = mpcekf_mex('ekf', h, vk, ik, tk)               mpcekf_ekf_step     (iterEKF.m:30)
 *   lin               = mpcekf_mex('linearize', h, zk, xm, xg, tk)     mpcekf_linearize    (EKFmatsHandler.m:1)
 *   [uk,nexec,J_uncon,J_final,norm_DU,viol] = mpcekf_mex('mpc', h, lin, soc_k1)
 *                                                                      mpcekf_mpc_step_ex  (iterMPC.m:1,89-95)
 *   [poles,sv]        = mpcekf_mex('mpcdiag', h, lin, uk_1)            mpcekf_mpc_diag     (iterMPC.m:53-60)
 *                       uk_1: [] for the context's; poles complex 7 x ncells, sv 7 x ncells
 *   [DU,lambda,nexec] = mpcekf_mex('hildreth', E, F, M, gamma, lambda0, maxIter)   (hildreth.m:1)
 *   [Phi,G]           = mpcekf_mex('predmat', a, C, D, Np, Nc)         (predMat.m:1, A = diag(a), B = 1)
 *   st                = mpcekf_mex('get_state', h)    /  mpcekf_mex('set_state', h, st)
 *                       st.bigX, ekf, scal, lambda (double), warn, status (int32 1 x ncells),
 *                       and st.mb (42 x ncells) on a model-blend ('MB') context (optional
 *                       in set_state: a checkpoint without it keeps the blend state)
 *   [s,warn,status]   = mpcekf_mex('scalars', h, idx)                 mpcekf_get_scalars
 *                       s: numel(idx) x ncells of the 1-based MPCEKF_S_* slots idx (1-2
 *                       SOCnAvg/SOCpAvg, 3 x0, 4 SigmaX0, 5 priorI, 6 uk_1, 7 uk, 8 vk):
 *                       what the drop-ins read every step, 8 B per slot and cell
 *                       mpcekf_mex('graph', h, enable)                 mpcekf_set_graph (replay repeated step calls)
 *                       mpcekf_mex('setlimits', h, idx, values)        mpcekf_set_limits (runMPC.m:30-44 per cell)
 *                       idx: 1-based MPCEKF_LIM_* field numbers (1 target_soc, 2 Crate, 3 u_max,
 *                       4 du_min, 5 du_max, 6 v_max, 7 phise_min, 8 z_max, 9 z_tol), each once;
 *                       values: ncells x numel(idx), column j = field idx(j) of every cell, in
 *                       the cfg struct's units.  A field not named keeps what it had
 *   values            = mpcekf_mex('getlimits', h, idx)                mpcekf_get_limits
 *                       ncells x numel(idx): what 'setlimits' stored, else the cfg scalar
 *                       mpcekf_mex('clearlimits', h)                   mpcekf_clear_limits
 *                       mpcekf_mex('summarybegin', h, reach, slot)     mpcekf_summary_begin
 *                       reach: [] or ncells SOC thresholds (the unit of 'step's soc: a fraction
 *                       0..1); slot: [] or 0 for none, else one 1-based slot of the obs record
 *                       mpcekf_mex('stepsummary', h, nsteps, tc)       mpcekf_step_summary
 *                       'step' without outputs, folded into the per-cell summary record
 *   s                 = mpcekf_mex('getsummary', h)                    mpcekf_get_summary
 *                       struct of ncells x 1 column vectors, one per MPCEKF_SUM_* field
 *                       (seen, steps, err_step, t_reach, u_min, ...; include/mpcekf.h)
 *                       mpcekf_mex('summaryend', h)                    mpcekf_summary_end
 *                       mpcekf_mex('thermalbegin', h, params, ocv, t0) mpcekf_thermal_begin
 *                       params: ncells x 3, columns Cth (J/K), Rth (K/W, Inf: adiabatic), Tamb
 *                       (degC); ocv: the open-circuit voltage on a uniform cell-SOC grid 0..1
 *                       (2 entries or more); t0: [] (keep) or ncells temperatures (degC).  From
 *                       then on every 'step' / 'stepobs' / 'stepsummary' / 'stepthermal' advances
 *                       each cell's temperature after every step and takes no tc
 *   s                 = mpcekf_mex('thermalget', h)                    mpcekf_thermal_get
 *                       struct of ncells x 1 column vectors: T, T_max, T_max_step, T_min,
 *                       heat_sum, steps, nheld (MPCEKF_THR_*; include/mpcekf.h)
 *                       mpcekf_mex('thermalend', h)                    mpcekf_thermal_end
 *   [u,v,soc,phise,nexec,temp,heat] = mpcekf_mex('stepthermal', h, nsteps)   mpcekf_step_ex_thermal
 *                       'step' on a context with a thermal model, plus the temperature each
 *                       step used and the heat it generated (W), ncells x nsteps
 *                       mpcekf_mex('thermalschedule', h, idx, T_lo, T_hi, tables, sets)   mpcekf_thermal_schedule
 *                       MPC limits that follow the model's temperature.  idx: 1-based field numbers
 *                       as in 'setlimits', each once, among 2 Crate, 3 u_max, 4 du_min, 5 du_max,
 *                       6 v_max, 7 phise_min; T_lo < T_hi: the uniform grid's ends (degC); tables:
 *                       ntab x numel(idx) x nsets (or ntab x numel(idx)*nsets), ntab >= 2, column
 *                       (j, s) = field idx(j) of derating map s over the grid; sets: [] (map 1) or
 *                       ncells 1-based map numbers.  'getlimits' then returns the values in force
 *                       mpcekf_mex('thermalscheduleend', h)            mpcekf_thermal_schedule_end
 *                       mpcekf_mex('limitmap', h, idx, z_lo, z_hi, T_lo, T_hi, tables, interp, sets, z0)   mpcekf_limit_map
 *                       MPC limits that follow each cell's SOC estimate and temperature.  idx: as
 *                       'thermalschedule'; z_lo < z_hi: the SOC grid's ends (fractions); T_lo < T_hi:
 *                       the temperature grid's ends (degC; [] without a temperature axis); tables:
 *                       nz x nt x numel(idx) x nsets (trailing dimensions may be folded), entry
 *                       (jz, jt, j, s) = field idx(j) of map s at SOC node jz and temperature node
 *                       jt; nt >= 2 needs 'thermalbegin'; interp: 0 / [] linear in SOC, 1 hold (the
 *                       left node's value); sets: [] (map 1) or ncells 1-based map numbers; z0: []
 *                       or ncells SOC fractions to evaluate at before the first fused step
 *   s                 = mpcekf_mex('limitmapget', h)                   mpcekf_limit_map_get
 *                       struct of ncells x 1 column vectors: z_last, neval, nclamp_z, nclamp_t (MPCEKF_LM_*)
 *                       mpcekf_mex('limitmapend', h)                   mpcekf_limit_map_end
 *   [u,v,soc,phise,nexec,lim] = mpcekf_mex('stepexmap', h, nsteps[, tc])   mpcekf_step_ex_map
 *                       'step' on a context with a limit map, plus the mapped fields' values the
 *                       MPC stage of every step read, ncells x (numel(idx)*nsteps),
 *                       column (j, t) = field idx(j) at step t
 *                       mpcekf_mex('thermalcouple', h, r_link)         mpcekf_thermal_couple
 *                       heat conduction between neighbouring cells of a pack string (needs
 *                       'thermalbegin' and 'packbegin'): r_link, ncells resistances (K/W, Inf: no
 *                       link) between cell c and c+1, used where both are in one string
 *   s                 = mpcekf_mex('thermalcoupleget', h)              mpcekf_thermal_couple_get
 *                       struct of ncells x 1 column vectors: nb_sum, dt_max, dt_max_step (MPCEKF_TCR_*)
 *                       mpcekf_mex('thermalcoupleend', h)              mpcekf_thermal_couple_end
 *   [u,v,soc,phise,nexec,temp,heat,cond] = mpcekf_mex('stepexcouple', h, nsteps)   mpcekf_step_ex_couple
 *                       'stepthermal' on a context with links, plus the heat each cell's
 *                       neighbours conducted to it in every step (W), ncells x nsteps
 *                       mpcekf_mex('packbegin', h, series)             mpcekf_pack_begin
 *                       the cells form ncells / series strings of `series` cells in series (cells
 *                       (g-1)*series+1 .. g*series are string g); from then on every 'step' /
 *                       'stepobs' / 'stepsummary' / 'stepthermal' / 'stepexpack' applies to each
 *                       cell its string's current, the largest command among the string's cells
 *   s                 = mpcekf_mex('packget', h)                       mpcekf_pack_get
 *                       struct of ncells x 1 column vectors: nlim, steps, headroom (MPCEKF_PK_*)
 *                       mpcekf_mex('packend', h)                       mpcekf_pack_end
 *   [u,v,soc,phise,nexec,ucmd,limiter] = mpcekf_mex('stepexpack', h, nsteps[, tc])   mpcekf_step_ex_pack
 *                       'step' on a pack context (u: the applied current), plus each cell's own
 *                       command, ncells x nsteps, and each string's limiter, nstrings x nsteps
 *                       int32, the 1-based in-string index or 0 for a string with no command
 *                       mpcekf_mex('agingbegin', h, params, sources)   mpcekf_aging_begin
 *                       side reactions (plating, SEI) integrated per cell after every fused step.
 *                       params: ncells x 5 x nreact (nreact 1..4), columns i0 (A), U (V), alpha,
 *                       Ea (J/mol), gate (V, Inf: always on); sources: 1 the EKF's phise, 2 the
 *                       plant's negPhise0, 3 both
 *   s                 = mpcekf_mex('agingget', h, source, react)       mpcekf_aging_get
 *                       struct of ncells x 1 column vectors: q_sum, j_max, j_max_step, n_on, steps,
 *                       nskip (MPCEKF_AGR_*) of source 1 or 2 and the 1-based reaction react
 *                       mpcekf_mex('agingend', h)                      mpcekf_aging_end
 *   [u,v,soc,phise,nexec,rate] = mpcekf_mex('stepexaging', h, nsteps[, tc])   mpcekf_step_ex_aging
 *                       'step' on an aging context, plus every step's side-reaction currents (A),
 *                       ncells x (nsrc*nreact) x nsteps: the enabled sources in order, reactions inside
 *                       mpcekf_mex('termbegin', h, params, hold)       mpcekf_term_begin
 *                       charge termination: params ncells x 3, columns soc_stop (a fraction 0..1),
 *                       i_taper (A), T_cut (degC), NaN: that criterion off; hold: the steps the
 *                       current stays at or under i_taper.  From then on every fused step latches
 *                       the cells that meet a criterion and rests them at 0 A
 *   s                 = mpcekf_mex('termget', h)                       mpcekf_term_get
 *                       struct of ncells x 1 column vectors: state (0 open, 1 latched, 2 dead),
 *                       done_step, reason, soc_done, u_done, T_done, rest, steps (MPCEKF_TM_*)
 *                       mpcekf_mex('termend', h)                       mpcekf_term_end
 *                       mpcekf_mex('balancebegin', h, params, compensate)   mpcekf_balance_begin
 *                       passive balancing on a pack ('packbegin' first): params ncells x 3, columns
 *                       i_bleed (A, >= 0), dz_on (a SOC fraction > 0), dz_off (0 .. dz_on);
 *                       compensate 0 / 1: the charger adds a bleeding cell's bleed current.  From then
 *                       on every fused step bleeds the cells that are dz_on above their string's
 *                       smallest soc
 *   s                 = mpcekf_mex('balanceget', h)                    mpcekf_balance_get
 *                       struct of ncells x 1 column vectors: steps_on, q_bleed, switches, dz_max,
 *                       dz_last, steps (MPCEKF_BL_*)
 *                       mpcekf_mex('balanceend', h)                    mpcekf_balance_end
 *   [u,v,soc,phise,nexec,ucmd,limiter,bleed,zmin] = mpcekf_mex('stepexbalance', h, nsteps[, tc])
 *                       mpcekf_step_ex_balance:
 *                       'stepexpack' on a context with a balancer, plus each cell's bleed current,
 *                       ncells x nsteps, and each string's smallest soc, nstrings x nsteps
 *                       mpcekf_mex('chargerbegin', h, params)          mpcekf_charger_begin
 *                       a charger's ratings on a pack ('packbegin' first; with or without a balancer):
 *                       params nstrings x 2, columns i_max (A, >= 0) and p_max (W, > 0), NaN: that cap
 *                       is off.  From then on every fused step adds up each string's voltage and
 *                       raises its charging current to -i_max and -p_max / V where those are larger
 *   s                 = mpcekf_mex('chargerget', h)                    mpcekf_charger_get
 *                       struct of nstrings x 1 column vectors: steps, ncap_i, ncap_p, q, e, curtail,
 *                       p_min, v_peak, nvalid_min (MPCEKF_CH_*)
 *                       mpcekf_mex('chargerend', h)                    mpcekf_charger_end
 *   [u,v,soc,phise,nexec,ucmd,limiter,bal,chg] = mpcekf_mex('stepexcharger', h, nsteps[, tc])
 *                       mpcekf_step_ex_charger:
 *                       'stepexpack' on a context with a charger (limiter: 1-based, 0 no command, -1 a
 *                       cap set the current), plus two structs: bal with bleed (ncells x nsteps) and
 *                       zmin (nstrings x nsteps), both [] on a context without a balancer; chg with
 *                       vstr, istr (nstrings x nsteps) and capby (int32: -1 no current, 0 not capped,
 *                       1 the current cap, 2 the power cap)
 *   [steps_run, open] = mpcekf_mex('stepuntil', h, max_steps, chunk[, tc])   mpcekf_step_until
 *                       fused steps in calls of `chunk` until no cell is open or max_steps are
 *                       run; tc: [] or ncells temperatures, the same for every step
 * Per-cell vectors are 1 x ncells or ncells x 1; zk / zbk are (nz+2) x ncells, xm / xg
 * 4 x ncells (xm: 0-based model index t*nZ+z), lin 35 x ncells -- MATLAB's column-major
 * k x ncells is the library's cell-major [ncells][k], so no copy is made for them.
 * Arrays the library reads row-major (the ROM's A/C/D, the electrode tables, hildreth's
 * E and M) are transposed here from MATLAB's column-major order.
 * Scalars (device, ncells, nsteps, cfg fields ...) may be of any real numeric class.
 * Only the first max(nargout, 1) outputs are returned.
 * Library failures raise a MATLAB error with mpcekf_last_error(); per-cell soft
 * failures stay in the status word (get_state), as in the C-ABI.
 * `clear mex` / MATLAB exit destroys every context still live (mexAtExit), freeing its
 * device memory; handles saved across a clear are then rejected as not live.
 */
#include <stdint.h>
#include <string.h>

#include "matrix.h"
#include "mex.h"
#include "mpcekf.h"

static void chk(int rc) {
  if (rc != MPCEKF_OK) mexErrMsgIdAndTxt("mpcekf:lib", "mpcekf error %d: %s", rc, mpcekf_last_error());
}

/* Live contexts of this MEX session: a handle is checked against them before use, so a
 * stale or made-up uint64 raises a MATLAB error instead of crashing MATLAB. */
#define MAXCTX 64
static mpcekf_ctx *g_live[MAXCTX];
static int32_t g_series[MAXCTX]; /* 'packbegin's series of g_live[i] (0: no pack): sizes 'stepexpack's limiter */
static int32_t g_agrows[MAXCTX]; /* 'agingbegin's nsrc * nreact of g_live[i] (0: none): sizes 'stepexaging's rate */
static int32_t g_mapnf[MAXCTX];  /* 'limitmap's numel(idx) of g_live[i] (0: none): sizes 'stepexmap's lim */

static void track(mpcekf_ctx *h, int add) {
  for (int i = 0; i < MAXCTX; ++i)
    if (add ? g_live[i] == NULL : g_live[i] == h) {
      g_live[i] = add ? h : NULL;
      g_series[i] = 0;
      g_agrows[i] = 0;
      g_mapnf[i] = 0;
      return;
    }
}

/* mexAtExit: `clear mex` or MATLAB exit releases every live context's device memory */
static void destroy_all(void) {
  for (int i = 0; i < MAXCTX; ++i)
    if (g_live[i]) {
      (void)mpcekf_ctx_destroy(g_live[i]);
      g_live[i] = NULL;
      g_series[i] = 0;
      g_agrows[i] = 0;
      g_mapnf[i] = 0;
    }
}

static int32_t *series_of(mpcekf_ctx *h) {
  for (int i = 0; i < MAXCTX; ++i)
    if (g_live[i] == h) return &g_series[i];
  return NULL;
}

static int32_t *agrows_of(mpcekf_ctx *h) {
  for (int i = 0; i < MAXCTX; ++i)
    if (g_live[i] == h) return &g_agrows[i];
  return NULL;
}

static int32_t *mapnf_of(mpcekf_ctx *h) {
  for (int i = 0; i < MAXCTX; ++i)
    if (g_live[i] == h) return &g_mapnf[i];
  return NULL;
}

static mpcekf_ctx *handle(const mxArray *a) {
  if (!mxIsUint64(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("mpcekf:arg", "expected a uint64 handle");
  mpcekf_ctx *h = (mpcekf_ctx *)(uintptr_t)(*(uint64_t *)mxGetData(a));
  for (int i = 0; i < MAXCTX; ++i)
    if (h && g_live[i] == h) return h;
  mexErrMsgIdAndTxt("mpcekf:arg", "not a live mpcekf context handle (destroyed, or not from 'create')");
  return NULL;
}

/* a real scalar of any numeric class (double, int32, ...), as MATLAB code passes them */
static double scalar(const mxArray *a, const char *what) {
  if (!a || !mxIsNumeric(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != 1)
    mexErrMsgIdAndTxt("mpcekf:arg", "%s: expected a real numeric scalar", what);
  return mxGetScalar(a);
}

/* an int32 array of exactly n elements (warn / status / xm) */
static int32_t *ivec(const mxArray *a, size_t n, const char *what) {
  if (!a || !mxIsInt32(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != n)
    mexErrMsgIdAndTxt("mpcekf:arg", "%s: expected %zu int32 values", what, n);
  return (int32_t *)mxGetData(a);
}

static const double *dvec(const mxArray *a, size_t n, const char *what) {
  if (!a || !mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != n)
    mexErrMsgIdAndTxt("mpcekf:arg", "%s: expected %zu real doubles", what, n);
  return mxGetDoubles(a);
}

/* MATLAB column-major N-D array -> C row-major copy (same dims) */
static double *rowmajor(const mxArray *a, const char *what) {
  if (!a || !mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("mpcekf:arg", "%s: expected a real double array", what);
  const mwSize nd = mxGetNumberOfDimensions(a);
  const mwSize *dims = mxGetDimensions(a);
  const size_t n = mxGetNumberOfElements(a);
  const double *src = mxGetDoubles(a);
  double *dst = (double *)mxMalloc(n * sizeof(double) + 8);
  mwSize idx[8] = {0};
  if (nd > 8) mexErrMsgIdAndTxt("mpcekf:arg", "%s: too many dimensions", what);
  for (size_t lin = 0; lin < n; ++lin) { /* lin walks the row-major order; idx its subscripts */
    size_t cm = 0, stride = 1;
    for (mwSize d = 0; d < nd; ++d) {
      cm += idx[d] * stride;
      stride *= dims[d];
    }
    dst[lin] = src[cm];
    for (mwSize d = nd; d-- > 0;) {
      if (++idx[d] < dims[d]) break;
      idx[d] = 0;
    }
  }
  return dst;
}

static const mxArray *field(const mxArray *s, const char *name) {
  const mxArray *f = mxGetField(s, 0, name);
  if (!f) mexErrMsgIdAndTxt("mpcekf:arg", "struct: missing field %s", name);
  return f;
}

/* ABI v3 (optional): e.poly.{Uocp,dUocp,k0,Rf,Cdleff} ntemp x (ntheta-1) x npoly and
 * e.poly.Uocp1 (ntheta-1) x npoly theta polynomials; e.Ea 1 x 5 Arrhenius energies (J/mol)
 * of Uocp, dUocp, k0, Rf, Cdleff.  Returns npoly (0: no polynomials). */
static int electrode_v3(const mxArray *e, mpcekf_electrode *out, int ntemp, int ntheta) {
  const mxArray *ea = mxGetField(e, 0, "Ea");
  if (ea && !mxIsEmpty(ea)) {
    const double *v = dvec(ea, 5, "Ea");
    for (int i = 0; i < 5; ++i) out->Ea[i] = v[i];
  }
  const mxArray *p = mxGetField(e, 0, "poly");
  if (!p || mxIsEmpty(p)) return 0;
  if (!mxIsStruct(p)) mexErrMsgIdAndTxt("mpcekf:arg", "poly: expected a struct");
  const mxArray *u1 = field(p, "Uocp1");
  const int np = (int)mxGetN(u1);
  if ((np != 4 && np != 6) || mxGetM(u1) != (size_t)(ntheta - 1))
    mexErrMsgIdAndTxt("mpcekf:arg", "poly.Uocp1: expected (ntheta-1) x 4 or x 6");
  out->Uocp1_p = rowmajor(u1, "poly.Uocp1");
  const char *names[5] = {"Uocp", "dUocp", "k0", "Rf", "Cdleff"};
  const double **dst[5] = {&out->Uocp_p, &out->dUocp_p, &out->k0_p, &out->Rf_p, &out->Cdleff_p};
  for (int i = 0; i < 5; ++i) {
    const mxArray *t = field(p, names[i]);
    if (mxGetNumberOfElements(t) != (size_t)ntemp * (ntheta - 1) * np)
      mexErrMsgIdAndTxt("mpcekf:arg", "poly.%s: expected ntemp x (ntheta-1) x %d", names[i], np);
    *dst[i] = rowmajor(t, names[i]);
  }
  return np;
}

/* ABI v4 (optional): e.nodes.{Uocp,dUocp,k0,Rf,Cdleff,Uocp1}, each a struct with x (1 x m
 * ascending theta nodes) and p (ntemp x (m-1) x npoly; Uocp1 (m-1) x npoly) -- a function
 * on its own breakpoints (include/mpcekf.h nnode / node / node_p; mpcekf_build_tables fills
 * them for lookup-table handles).  npoly must be the poly tables' (tab_npoly). */
static void electrode_v4(const mxArray *e, mpcekf_electrode *out, int ntemp, int npoly) {
  const mxArray *nd = mxGetField(e, 0, "nodes");
  if (!nd || mxIsEmpty(nd)) return;
  if (!mxIsStruct(nd)) mexErrMsgIdAndTxt("mpcekf:arg", "nodes: expected a struct");
  if (!npoly) mexErrMsgIdAndTxt("mpcekf:arg", "nodes: needs the poly tables (ABI v3) beside them");
  const char *names[6] = {"Uocp", "dUocp", "k0", "Rf", "Cdleff", "Uocp1"};
  for (int f = 0; f < 6; ++f) {
    const mxArray *t = mxGetField(nd, 0, names[f]);
    if (!t || mxIsEmpty(t)) continue;
    const mxArray *x = field(t, "x"), *p = field(t, "p");
    const size_t m = mxGetNumberOfElements(x);
    const size_t rows = f == 5 ? 1 : (size_t)ntemp;
    if (m < 2 || mxGetNumberOfElements(p) != rows * (m - 1) * (size_t)npoly)
      mexErrMsgIdAndTxt("mpcekf:arg", "nodes.%s: x needs >= 2 nodes and p %s x (m-1) x %d", names[f],
                        f == 5 ? "1" : "ntemp", npoly);
    out->nnode[f] = (int32_t)m;
    out->node[f] = dvec(x, m, names[f]);
    out->node_p[f] = rowmajor(p, names[f]);
  }
}

static void electrode(const mxArray *e, mpcekf_electrode *out, int ntemp, int ntheta) {
  out->theta0 = scalar(field(e, "theta0"), "theta0");
  out->theta100 = scalar(field(e, "theta100"), "theta100");
  out->soc0 = dvec(field(e, "soc0"), (size_t)ntemp, "soc0");
  out->soc100 = dvec(field(e, "soc100"), (size_t)ntemp, "soc100");
  out->Uocp1 = dvec(field(e, "Uocp1"), (size_t)ntheta, "Uocp1");
  const char *names[5] = {"Uocp", "dUocp", "k0", "Rf", "Cdleff"};
  const double **dst[5] = {&out->Uocp, &out->dUocp, &out->k0, &out->Rf, &out->Cdleff};
  for (int i = 0; i < 5; ++i) { /* ntemp x ntheta in MATLAB -> [ntemp][ntheta] */
    const mxArray *t = field(e, names[i]);
    if (mxGetNumberOfElements(t) != (size_t)ntemp * ntheta) mexErrMsgIdAndTxt("mpcekf:arg", "%s: size", names[i]);
    *dst[i] = rowmajor(t, names[i]);
  }
}

static void rom_from_struct(const mxArray *R, mpcekf_rom *r) {
  memset(r, 0, sizeof(*r));
  const mxArray *A = field(R, "A"), *C = field(R, "C");
  const mwSize *da = mxGetDimensions(A), *dc = mxGetDimensions(C);
  if (mxGetNumberOfDimensions(A) != 3 || mxGetNumberOfDimensions(C) != 4)
    mexErrMsgIdAndTxt("mpcekf:arg", "ROM: A must be nT x nZ x (n+1), C nT x nZ x nz x (n+1)");
  r->nT = (int32_t)da[0];
  r->nZ = (int32_t)da[1];
  r->n = (int32_t)da[2] - 1;
  r->nz = (int32_t)dc[2];
  r->T_degC = dvec(field(R, "T_degC"), (size_t)r->nT, "T_degC");
  r->SOC_pct = dvec(field(R, "SOC_pct"), (size_t)r->nZ, "SOC_pct");
  r->Ts = scalar(field(R, "Ts"), "Ts");
  r->A = rowmajor(A, "A");
  r->C = rowmajor(C, "C");
  r->D = rowmajor(field(R, "D"), "D");
  const mxArray *code = field(R, "tf_code");
  if (!mxIsInt32(code) || mxGetNumberOfElements(code) != (size_t)r->nz) mexErrMsgIdAndTxt("mpcekf:arg", "tf_code: int32 x nz");
  r->tf_code = (const int32_t *)mxGetData(code);
  r->tf_xloc = dvec(field(R, "xloc"), (size_t)r->nz, "xloc");
  r->F = scalar(field(R, "F"), "F");
  r->R = scalar(field(R, "R"), "R");
  r->Q = scalar(field(R, "Q"), "Q");
  r->Rc = scalar(field(R, "Rc"), "Rc");
  r->Tref = scalar(field(R, "Tref"), "Tref");
  const mxArray *TK = field(R, "tab_T_K");
  r->tab_ntemp = (int32_t)mxGetNumberOfElements(TK);
  r->tab_T_K = dvec(TK, (size_t)r->tab_ntemp, "tab_T_K");
  r->tab_ntheta = (int32_t)mxGetNumberOfElements(field(field(R, "neg"), "Uocp1"));
  electrode(field(R, "neg"), &r->neg, r->tab_ntemp, r->tab_ntheta);
  electrode(field(R, "pos"), &r->pos, r->tab_ntemp, r->tab_ntheta);
  const int npn = electrode_v3(field(R, "neg"), &r->neg, r->tab_ntemp, r->tab_ntheta);
  const int npp = electrode_v3(field(R, "pos"), &r->pos, r->tab_ntemp, r->tab_ntheta);
  if (npn != npp) mexErrMsgIdAndTxt("mpcekf:arg", "ROM: poly tables for both electrodes or neither, same order");
  r->tab_npoly = npn;
  electrode_v4(field(R, "neg"), &r->neg, r->tab_ntemp, npn);
  electrode_v4(field(R, "pos"), &r->pos, r->tab_ntemp, npn);
}

static void cfg_from_struct(const mxArray *s, mpcekf_config *c) {
  mpcekf_config_defaults(c);
  if (!s || mxIsEmpty(s)) return;
  if (!mxIsStruct(s)) mexErrMsgIdAndTxt("mpcekf:arg", "cfg: expected a struct");
#define GETI(f) if (mxGetField(s, 0, #f)) c->f = (int32_t)scalar(mxGetField(s, 0, #f), #f)
#define GETD(f) if (mxGetField(s, 0, #f)) c->f = scalar(mxGetField(s, 0, #f), #f)
  GETI(Np); GETI(Nc); GETD(target_soc); GETD(Crate); GETD(u_max); GETD(du_min); GETD(du_max); GETD(v_min);
  GETD(v_max); GETD(phise_min); GETD(z_max); GETD(z_tol); GETI(use_current); GETI(use_voltage); GETI(use_eta);
  GETI(max_hild); GETD(hild_tol); GETD(SigmaV); GETD(SigmaW); GETI(max_warn); GETI(flags); GETI(method);
#undef GETI
#undef GETD
  if (c->method != MPCEKF_METHOD_OB && c->method != MPCEKF_METHOD_MB)
    mexErrMsgIdAndTxt("mpcekf:arg", "cfg.method: %d (expected 0 = 'OB' or 1 = 'MB', initKF.m:44-49)", (int)c->method);
  const mxArray *sx = mxGetField(s, 0, "SigmaX0");
  if (sx) {
    const double *v = dvec(sx, 6, "SigmaX0 (diagonal, 6)");
    for (int i = 0; i < 6; ++i) c->SigmaX0[i] = v[i];
  }
}

/* a real double N-D array ('stepobs': ncells x nslots x nsteps).  The MEX API test shim this
 * gateway is also built against (tests/mex, not MATLAB) declares no N-D constructor; the entry
 * point its driver makes arrays with serves there, trailing singletons dropped as MATLAB does. */
#ifdef MPCEKF_TEST_MATRIX_H
mxArray *shim_numeric(int cls, int nd, const size_t *dims, const void *data, int cplx);
static mxArray *dnd(mwSize nd, const mwSize *dims) {
  while (nd > 2 && dims[nd - 1] == 1) --nd;
  return shim_numeric((int)mxDOUBLE_CLASS, (int)nd, dims, NULL, 0);
}
#else
static mxArray *dnd(mwSize nd, const mwSize *dims) { return mxCreateNumericArray(nd, dims, mxDOUBLE_CLASS, mxREAL); }
#endif
static mxArray *dmat(size_t r, size_t c) { return mxCreateDoubleMatrix((mwSize)r, (mwSize)c, mxREAL); }
static mxArray *imat(size_t r, size_t c) { return mxCreateNumericMatrix((mwSize)r, (mwSize)c, mxINT32_CLASS, mxREAL); }

static const double *opt_vec(const mxArray *a, size_t n, const char *what) {
  return (!a || mxIsEmpty(a)) ? NULL : dvec(a, n, what);
}

/* Every command builds its outputs in plhs[0..MAXOUT); mexFunction hands MATLAB the
 * first max(nlhs, 1) of them (MATLAB's plhs has room for no more) and frees the rest. */
#define MAXOUT 9
static void need(int nrhs, int k, const char *usage) {
  if (nrhs < k) mexErrMsgIdAndTxt("mpcekf:arg", "usage: mpcekf_mex(%s)", usage);
}

static int g_nlhs = 1; /* the caller's nargout: 'ekf' copies Xind back only when it is asked for */
static void gateway(mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  char cmd[32];
  if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd)) mexErrMsgIdAndTxt("mpcekf:arg", "first argument: command");
  if (!strcmp(cmd, "create")) {
    if (nrhs != 5) mexErrMsgIdAndTxt("mpcekf:arg", "create(R, cfg, device, ncells)");
    mpcekf_rom r;
    mpcekf_config c;
    rom_from_struct(prhs[1], &r);
    cfg_from_struct(prhs[2], &c);
    int free_slot = 0;
    for (int i = 0; i < MAXCTX; ++i) free_slot = free_slot || g_live[i] == NULL;
    if (!free_slot) mexErrMsgIdAndTxt("mpcekf:arg", "create: %d contexts are live; destroy one first", MAXCTX);
    mpcekf_ctx *h = NULL;
    chk(mpcekf_ctx_create(&r, &c, (int)scalar(prhs[3], "device"), (int64_t)scalar(prhs[4], "ncells"), &h));
    track(h, 1);
    mexAtExit(destroy_all);
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *(uint64_t *)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
    return; /* the row-major copies are mxMalloc'd: MATLAB frees them (the context copied the ROM) */
  }
  if (!strcmp(cmd, "hildreth")) {
    if (nrhs != 7) mexErrMsgIdAndTxt("mpcekf:arg", "hildreth(E, F, M, gamma, lambda0, maxIter)");
    const size_t Nc = mxGetM(prhs[1]), nC = mxGetM(prhs[3]);
    if (mxGetNumberOfDimensions(prhs[1]) != 2 || mxGetN(prhs[1]) != Nc)
      mexErrMsgIdAndTxt("mpcekf:arg", "hildreth: E must be Nc x Nc");
    if (mxGetNumberOfDimensions(prhs[3]) != 2 || mxGetN(prhs[3]) != Nc)
      mexErrMsgIdAndTxt("mpcekf:arg", "hildreth: M must be nC x Nc (Nc = %zu)", Nc);
    double *E = rowmajor(prhs[1], "E"), *M = rowmajor(prhs[3], "M");
    const double *F = dvec(prhs[2], Nc, "F"), *g = dvec(prhs[4], nC, "gamma");
    plhs[1] = dmat(nC, 1);
    memcpy(mxGetDoubles(plhs[1]), dvec(prhs[5], nC, "lambda0"), nC * sizeof(double));
    plhs[0] = dmat(Nc, 1);
    mxArray *ne = imat(1, 1);
    chk(mpcekf_hildreth(0, 1, (int32_t)Nc, (int32_t)nC, E, F, M, g, mxGetDoubles(plhs[1]),
                        (int32_t)scalar(prhs[6], "maxIter"), 1e-6, mxGetDoubles(plhs[0]), (int32_t *)mxGetData(ne)));
    plhs[2] = mxCreateDoubleScalar((double)*(int32_t *)mxGetData(ne));
    mxDestroyArray(ne);
    return;
  }
  if (!strcmp(cmd, "predmat")) {
    if (nrhs != 6) mexErrMsgIdAndTxt("mpcekf:arg", "predmat(a, C, D, Np, Nc)");
    const int Np = (int)scalar(prhs[4], "Np"), Nc = (int)scalar(prhs[5], "Nc");
    double *P = (double *)mxMalloc((size_t)Np * 7 * sizeof(double)), *G = (double *)mxMalloc((size_t)Np * Nc * sizeof(double));
    chk(mpcekf_predmat(0, 1, Np, Nc, dvec(prhs[1], 6, "a"), dvec(prhs[2], 6, "C"), dvec(prhs[3], 1, "D"), P, G));
    plhs[0] = dmat((size_t)Np, 7);
    plhs[1] = dmat((size_t)Np, (size_t)Nc);
    for (int i = 0; i < Np; ++i) { /* row-major -> column-major */
      for (int k = 0; k < 7; ++k) mxGetDoubles(plhs[0])[i + (size_t)Np * k] = P[i * 7 + k];
      for (int k = 0; k < Nc; ++k) mxGetDoubles(plhs[1])[i + (size_t)Np * k] = G[i * Nc + k];
    }
    return;
  }
  static const char *const with_handle[] = {"destroy", "init", "step", "plant", "ekf", "linearize", "mpc",
                                            "graph", "mpcdiag", "get_state", "set_state", "scalars", "linfields",
                                            "plantobs", "obsslots", "obslayout", "stepobs", "setlimits", "getlimits",
                                            "clearlimits", "summarybegin", "stepsummary", "getsummary", "summaryend",
                                            "thermalbegin", "thermalget", "thermalend", "stepthermal",
                                            "thermalschedule", "thermalscheduleend",
                                            "limitmap", "limitmapget", "limitmapend", "stepexmap",
                                            "thermalcouple", "thermalcoupleget", "thermalcoupleend", "stepexcouple",
                                            "packbegin", "packget", "packend", "stepexpack",
                                            "agingbegin", "agingget", "agingend", "stepexaging",
                                            "termbegin", "termget", "termend", "stepuntil",
                                            "balancebegin", "balanceget", "balanceend", "stepexbalance",
                                            "chargerbegin", "chargerget", "chargerend", "stepexcharger"};
  int known = 0;
  for (size_t i = 0; i < sizeof with_handle / sizeof *with_handle; ++i) known = known || !strcmp(cmd, with_handle[i]);
  if (!known) mexErrMsgIdAndTxt("mpcekf:arg", "unknown command %s", cmd);
  if (nrhs < 2) mexErrMsgIdAndTxt("mpcekf:arg", "%s: missing handle", cmd);
  /* the obs commands refuse what no context can make valid before they look at the handle,
     and before any device work: the output count, and slot indices that are no 1-based integers */
  if (!strcmp(cmd, "plantobs") && g_nlhs > 2) mexErrMsgIdAndTxt("mpcekf:arg", "plantobs: at most 2 outputs [Vcell, obs]");
  const int stepobs = !strcmp(cmd, "stepobs");
  if (!strcmp(cmd, "obsslots") || stepobs) {
    if (!stepobs && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "obsslots: at most 1 output");
    if (stepobs && g_nlhs > 6) mexErrMsgIdAndTxt("mpcekf:arg", "stepobs: at most 6 outputs [u, v, soc, phise, nexec, obs]");
    if (stepobs) need(nrhs, 4, "'stepobs', h, nsteps, idx[, tc]");
    else need(nrhs, 3, "'obsslots', h, idx");
    const mxArray *ia = prhs[stepobs ? 3 : 2];
    const size_t k = mxGetNumberOfElements(ia);
    if (k < 1) mexErrMsgIdAndTxt("mpcekf:arg", "%s: idx: expected at least 1 slot index", cmd);
    const double *idx = dvec(ia, k, "idx");
    for (size_t j = 0; j < k; ++j)
      if (!(idx[j] >= 1 && idx[j] <= 2147483647.0) || idx[j] != (double)(int32_t)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "%s: idx(%zu) = %g is not a slot 1..nobs", cmd, j + 1, idx[j]);
  }
  /* the limits commands likewise: output count, field numbers 1..MPCEKF_NLIM, each once */
  const int setlim = !strcmp(cmd, "setlimits"), getlim = !strcmp(cmd, "getlimits");
  int32_t limf[MPCEKF_NLIM];
  size_t nlimf = 0;
  if (!strcmp(cmd, "clearlimits") && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "clearlimits: no output");
  if (setlim || getlim) {
    if (setlim && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "setlimits: no output");
    if (getlim && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "getlimits: at most 1 output");
    if (setlim) need(nrhs, 4, "'setlimits', h, idx, values");
    else need(nrhs, 3, "'getlimits', h, idx");
    nlimf = mxGetNumberOfElements(prhs[2]);
    if (nlimf < 1 || nlimf > MPCEKF_NLIM)
      mexErrMsgIdAndTxt("mpcekf:arg", "%s: idx: expected 1..%d field numbers", cmd, (int)MPCEKF_NLIM);
    const double *idx = dvec(prhs[2], nlimf, "idx");
    unsigned seen = 0;
    for (size_t j = 0; j < nlimf; ++j) {
      if (!(idx[j] >= 1 && idx[j] <= MPCEKF_NLIM) || idx[j] != (double)(int)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "%s: idx(%zu) = %g is not a field 1..%d", cmd, j + 1, idx[j], (int)MPCEKF_NLIM);
      limf[j] = (int32_t)idx[j] - 1;
      if (seen >> limf[j] & 1) mexErrMsgIdAndTxt("mpcekf:arg", "%s: idx(%zu) = %g is given twice", cmd, j + 1, idx[j]);
      seen |= 1u << limf[j];
    }
    if (setlim && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "setlimits: values: expected a real double ncells x %zu array", nlimf);
  }
  /* the summary commands likewise: output count, argument classes, a slot that is no 1-based
     integer (0 / []: none), an nsteps that is no non-negative integer */
  const int sumbegin = !strcmp(cmd, "summarybegin"), stepsum = !strcmp(cmd, "stepsummary");
  int32_t sumslot = -1, sumsteps = 0;
  if (sumbegin || stepsum || !strcmp(cmd, "summaryend")) {
    if (g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  }
  if (!strcmp(cmd, "getsummary") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "getsummary: at most 1 output");
  if (sumbegin) {
    if (nrhs > 2 && !mxIsEmpty(prhs[2]) && (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2])))
      mexErrMsgIdAndTxt("mpcekf:arg", "summarybegin: reach: expected [] or ncells real doubles");
    if (nrhs > 3 && !mxIsEmpty(prhs[3])) {
      const double sd = scalar(prhs[3], "summarybegin: slot");
      if (!(sd >= 0 && sd <= 2147483647.0) || sd != (double)(int32_t)sd)
        mexErrMsgIdAndTxt("mpcekf:arg", "summarybegin: slot = %g is not a slot 1..nobs (0 or []: none)", sd);
      sumslot = (int32_t)sd - 1;
    }
  }
  if (stepsum) {
    need(nrhs, 3, "'stepsummary', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    sumsteps = (int32_t)nsd;
  }
  /* the thermal commands likewise: output count, argument classes, a table of 2 entries or
     more, an nsteps that is no non-negative integer */
  const int thbegin = !strcmp(cmd, "thermalbegin"), stepth = !strcmp(cmd, "stepthermal");
  int32_t thsteps = 0;
  if ((thbegin || !strcmp(cmd, "thermalend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "thermalget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "thermalget: at most 1 output");
  if (stepth && g_nlhs > 7)
    mexErrMsgIdAndTxt("mpcekf:arg", "stepthermal: at most 7 outputs [u, v, soc, phise, nexec, temp, heat]");
  if (thbegin) {
    need(nrhs, 4, "'thermalbegin', h, params, ocv[, t0]");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalbegin: params: expected a real double ncells x %d array", (int)MPCEKF_NTH);
    if (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3]) || mxGetNumberOfElements(prhs[3]) < 2 ||
        mxGetNumberOfElements(prhs[3]) > 2147483647.0)
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalbegin: ocv: expected 2 or more real doubles");
    if (nrhs > 4 && !mxIsEmpty(prhs[4]) && (!mxIsDouble(prhs[4]) || mxIsComplex(prhs[4])))
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalbegin: t0: expected [] or ncells real doubles");
  }
  if (stepth) {
    need(nrhs, 3, "'stepthermal', h, nsteps");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    thsteps = (int32_t)nsd;
  }
  /* the schedule commands likewise: output count, field numbers among the schedulable ones,
     each once, grid ends that are real scalars, tables of ntab >= 2 rows and a whole number of
     maps, set numbers that are 1-based integers */
  const int thsched = !strcmp(cmd, "thermalschedule");
  int32_t schf[MPCEKF_NLIM];
  size_t nschf = 0, schtab = 0, schsets = 0;
  double sch_lo = 0, sch_hi = 0;
  if ((thsched || !strcmp(cmd, "thermalscheduleend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (thsched) {
    need(nrhs, 6, "'thermalschedule', h, idx, T_lo, T_hi, tables[, sets]");
    nschf = mxGetNumberOfElements(prhs[2]);
    if (nschf < 1 || nschf > 6) mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: idx: expected 1..6 field numbers");
    const double *idx = dvec(prhs[2], nschf, "idx");
    unsigned seen = 0;
    for (size_t j = 0; j < nschf; ++j) {
      if (!(idx[j] >= MPCEKF_LIM_CRATE + 1 && idx[j] <= MPCEKF_LIM_PHISE_MIN + 1) || idx[j] != (double)(int)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: idx(%zu) = %g is not a field that can be scheduled (%d..%d)", j + 1,
                          idx[j], (int)MPCEKF_LIM_CRATE + 1, (int)MPCEKF_LIM_PHISE_MIN + 1);
      schf[j] = (int32_t)idx[j] - 1;
      if (seen >> schf[j] & 1) mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: idx(%zu) = %g is given twice", j + 1, idx[j]);
      seen |= 1u << schf[j];
    }
    sch_lo = scalar(prhs[3], "thermalschedule: T_lo");
    sch_hi = scalar(prhs[4], "thermalschedule: T_hi");
    if (!mxIsDouble(prhs[5]) || mxIsComplex(prhs[5]) || mxIsEmpty(prhs[5]))
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: tables: expected a real double ntab x %zu x nsets array", nschf);
    schtab = mxGetM(prhs[5]);
    const size_t cols = mxGetNumberOfElements(prhs[5]) / schtab;
    if (schtab < 2 || schtab > 2147483647.0 || cols % nschf != 0 || cols / nschf > 2147483647.0)
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: tables: %zu x %zu: expected ntab >= 2 rows and %zu columns per map",
                        schtab, cols, nschf);
    schsets = cols / nschf;
    if (nrhs > 6 && !mxIsEmpty(prhs[6])) {
      if (!mxIsDouble(prhs[6]) || mxIsComplex(prhs[6]))
        mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: sets: expected [] or ncells real doubles");
      const size_t k = mxGetNumberOfElements(prhs[6]);
      const double *sd = mxGetDoubles(prhs[6]);
      for (size_t j = 0; j < k; ++j)
        if (!(sd[j] >= 1 && sd[j] <= (double)schsets) || sd[j] != (double)(int32_t)sd[j])
          mexErrMsgIdAndTxt("mpcekf:arg", "thermalschedule: sets(%zu) = %g is not a map 1..%zu", j + 1, sd[j], schsets);
    }
  }
  /* the limit map's commands likewise: output count, field numbers among the mappable ones, each
     once, grid ends that are real scalars, tables of whole maps, an interp that is 0 or 1, set
     numbers that are 1-based integers, an nsteps that is no non-negative integer */
  const int lmset = !strcmp(cmd, "limitmap"), steplm = !strcmp(cmd, "stepexmap");
  int32_t lmf[MPCEKF_NLIM], lmsteps = 0, lminterp = 0;
  size_t nlmf = 0, lmnz = 0, lmnt = 0, lmsets = 0;
  double lm_zlo = 0, lm_zhi = 0, lm_tlo = 0, lm_thi = 1;
  if ((lmset || !strcmp(cmd, "limitmapend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "limitmapget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "limitmapget: at most 1 output");
  if (steplm && g_nlhs > 6) mexErrMsgIdAndTxt("mpcekf:arg", "stepexmap: at most 6 outputs [u, v, soc, phise, nexec, lim]");
  if (lmset) {
    need(nrhs, 8, "'limitmap', h, idx, z_lo, z_hi, T_lo, T_hi, tables[, interp[, sets[, z0]]]");
    nlmf = mxGetNumberOfElements(prhs[2]);
    if (nlmf < 1 || nlmf > 6) mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: idx: expected 1..6 field numbers");
    const double *idx = dvec(prhs[2], nlmf, "idx");
    unsigned seen = 0;
    for (size_t j = 0; j < nlmf; ++j) {
      if (!(idx[j] >= MPCEKF_LIM_CRATE + 1 && idx[j] <= MPCEKF_LIM_PHISE_MIN + 1) || idx[j] != (double)(int)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: idx(%zu) = %g is not a field that can be mapped (%d..%d)", j + 1, idx[j],
                          (int)MPCEKF_LIM_CRATE + 1, (int)MPCEKF_LIM_PHISE_MIN + 1);
      lmf[j] = (int32_t)idx[j] - 1;
      if (seen >> lmf[j] & 1) mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: idx(%zu) = %g is given twice", j + 1, idx[j]);
      seen |= 1u << lmf[j];
    }
    lm_zlo = scalar(prhs[3], "limitmap: z_lo");
    lm_zhi = scalar(prhs[4], "limitmap: z_hi");
    if (!mxIsDouble(prhs[7]) || mxIsComplex(prhs[7]) || mxIsEmpty(prhs[7]))
      mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: tables: expected a real double nz x nt x %zu x nsets array", nlmf);
    lmnz = mxGetM(prhs[7]);
    lmnt = mxGetNumberOfDimensions(prhs[7]) >= 2 ? mxGetDimensions(prhs[7])[1] : 1;
    const size_t rest = mxGetNumberOfElements(prhs[7]) / (lmnz * lmnt);
    if (lmnz > 2147483647.0 || lmnt > 2147483647.0 || (lmnz == 1 && lmnt == 1) || rest % nlmf != 0 ||
        rest / nlmf > 2147483647.0)
      mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: tables: %zu x %zu x %zu: expected 2 or more nodes on one axis and %zu "
                        "tables per map", lmnz, lmnt, rest, nlmf);
    lmsets = rest / nlmf;
    if (lmnt > 1 || !mxIsEmpty(prhs[5])) lm_tlo = scalar(prhs[5], "limitmap: T_lo");
    if (lmnt > 1 || !mxIsEmpty(prhs[6])) lm_thi = scalar(prhs[6], "limitmap: T_hi");
    if (nrhs > 8 && !mxIsEmpty(prhs[8])) {
      const double d = scalar(prhs[8], "limitmap: interp");
      if (d != 0 && d != 1) mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: interp = %g: 0 (linear) or 1 (hold)", d);
      lminterp = (int32_t)d;
    }
    if (nrhs > 9 && !mxIsEmpty(prhs[9])) {
      if (!mxIsDouble(prhs[9]) || mxIsComplex(prhs[9]))
        mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: sets: expected [] or ncells real doubles");
      const size_t k = mxGetNumberOfElements(prhs[9]);
      const double *sd = mxGetDoubles(prhs[9]);
      for (size_t j = 0; j < k; ++j)
        if (!(sd[j] >= 1 && sd[j] <= (double)lmsets) || sd[j] != (double)(int32_t)sd[j])
          mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: sets(%zu) = %g is not a map 1..%zu", j + 1, sd[j], lmsets);
    }
    if (nrhs > 10 && !mxIsEmpty(prhs[10]) && (!mxIsDouble(prhs[10]) || mxIsComplex(prhs[10])))
      mexErrMsgIdAndTxt("mpcekf:arg", "limitmap: z0: expected [] or ncells real doubles");
  }
  if (steplm) {
    need(nrhs, 3, "'stepexmap', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    lmsteps = (int32_t)nsd;
    if (nrhs > 3 && !mxIsEmpty(prhs[3]) && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepexmap: tc: expected [] or ncells x nsteps real doubles");
  }
  /* the coupling commands likewise: output count, the links' class, an nsteps that is no
     non-negative integer */
  const int tcset = !strcmp(cmd, "thermalcouple"), steptc = !strcmp(cmd, "stepexcouple");
  int32_t tcsteps = 0;
  if ((tcset || !strcmp(cmd, "thermalcoupleend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "thermalcoupleget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "thermalcoupleget: at most 1 output");
  if (steptc && g_nlhs > 8)
    mexErrMsgIdAndTxt("mpcekf:arg", "stepexcouple: at most 8 outputs [u, v, soc, phise, nexec, temp, heat, cond]");
  if (tcset) {
    need(nrhs, 3, "'thermalcouple', h, r_link");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "thermalcouple: r_link: expected ncells real doubles");
  }
  if (steptc) {
    need(nrhs, 3, "'stepexcouple', h, nsteps");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    tcsteps = (int32_t)nsd;
  }
  /* the pack commands likewise: output count, a series that is no positive integer, an nsteps
     that is no non-negative integer, a tc of the wrong class */
  const int pkbegin = !strcmp(cmd, "packbegin"), steppk = !strcmp(cmd, "stepexpack");
  int32_t pkseries = 0, pksteps = 0;
  if ((pkbegin || !strcmp(cmd, "packend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "packget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "packget: at most 1 output");
  if (steppk && g_nlhs > 7)
    mexErrMsgIdAndTxt("mpcekf:arg", "stepexpack: at most 7 outputs [u, v, soc, phise, nexec, ucmd, limiter]");
  if (pkbegin) {
    need(nrhs, 3, "'packbegin', h, series");
    const double sd = scalar(prhs[2], "packbegin: series");
    if (!(sd >= 1 && sd <= 2147483647.0) || sd != (double)(int32_t)sd)
      mexErrMsgIdAndTxt("mpcekf:arg", "packbegin: series = %g is not a positive integer", sd);
    pkseries = (int32_t)sd;
  }
  if (steppk) {
    need(nrhs, 3, "'stepexpack', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    pksteps = (int32_t)nsd;
    if (nrhs > 3 && !mxIsEmpty(prhs[3]) && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepexpack: tc: expected [] or ncells x nsteps real doubles");
  }
  /* the aging commands likewise: output count, params that are no ncells x 5 x nreact doubles,
     sources outside 1..3, a source / react that is no index, an nsteps that is no count */
  const int agbegin = !strcmp(cmd, "agingbegin"), agget = !strcmp(cmd, "agingget"), stepag = !strcmp(cmd, "stepexaging");
  int32_t agreact = 0, agsrc = 0, agsteps = 0;
  if ((agbegin || !strcmp(cmd, "agingend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (agget && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "agingget: at most 1 output");
  if (stepag && g_nlhs > 6)
    mexErrMsgIdAndTxt("mpcekf:arg", "stepexaging: at most 6 outputs [u, v, soc, phise, nexec, rate]");
  if (agbegin) {
    need(nrhs, 4, "'agingbegin', h, params, sources");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxIsEmpty(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "agingbegin: params: expected a real double ncells x 5 x nreact array");
    const size_t rows = mxGetM(prhs[2]), cols = mxGetNumberOfElements(prhs[2]) / rows;
    if (cols % MPCEKF_NAGP != 0 || cols / MPCEKF_NAGP < 1 || cols / MPCEKF_NAGP > MPCEKF_AG_MAXREACT)
      mexErrMsgIdAndTxt("mpcekf:arg", "agingbegin: params: %zu x %zu: expected 5 columns per reaction, 1..4 reactions", rows,
                        cols);
    agreact = (int32_t)(cols / MPCEKF_NAGP);
    const double sd = scalar(prhs[3], "agingbegin: sources");
    if (!(sd >= 1 && sd <= 3) || sd != (double)(int32_t)sd)
      mexErrMsgIdAndTxt("mpcekf:arg", "agingbegin: sources = %g is not 1 (est), 2 (plant) or 3 (both)", sd);
    agsrc = (int32_t)sd;
  }
  if (agget) {
    need(nrhs, 4, "'agingget', h, source, react");
    const double sd = scalar(prhs[2], "agingget: source"), rd = scalar(prhs[3], "agingget: react");
    if (sd != 1 && sd != 2) mexErrMsgIdAndTxt("mpcekf:arg", "agingget: source = %g is not 1 (est) or 2 (plant)", sd);
    if (!(rd >= 1 && rd <= MPCEKF_AG_MAXREACT) || rd != (double)(int32_t)rd)
      mexErrMsgIdAndTxt("mpcekf:arg", "agingget: react = %g is not a reaction 1..4", rd);
    agsrc = (int32_t)sd;
    agreact = (int32_t)rd - 1;
  }
  if (stepag) {
    need(nrhs, 3, "'stepexaging', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    agsteps = (int32_t)nsd;
    if (nrhs > 3 && !mxIsEmpty(prhs[3]) && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepexaging: tc: expected [] or ncells x nsteps real doubles");
  }
  /* the termination commands likewise: output count, params that are no real doubles, a hold or
     chunk that is no positive integer, a max_steps that is no count, a tc of the wrong class */
  const int tmbegin = !strcmp(cmd, "termbegin"), until = !strcmp(cmd, "stepuntil");
  int32_t tmhold = 0, tmmax = 0, tmchunk = 0;
  if ((tmbegin || !strcmp(cmd, "termend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "termget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "termget: at most 1 output");
  if (until && g_nlhs > 2) mexErrMsgIdAndTxt("mpcekf:arg", "stepuntil: at most 2 outputs [steps_run, open]");
  if (tmbegin) {
    need(nrhs, 4, "'termbegin', h, params, hold");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "termbegin: params: expected ncells x 3 real doubles");
    const double hd = scalar(prhs[3], "termbegin: hold");
    if (!(hd >= 1 && hd <= 2147483647.0) || hd != (double)(int32_t)hd)
      mexErrMsgIdAndTxt("mpcekf:arg", "termbegin: hold = %g is not a positive integer", hd);
    tmhold = (int32_t)hd;
  }
  if (until) {
    need(nrhs, 4, "'stepuntil', h, max_steps, chunk[, tc]");
    const double md = scalar(prhs[2], "max_steps"), cd = scalar(prhs[3], "stepuntil: chunk");
    if (!(md >= 0 && md <= 2147483647.0) || md != (double)(int32_t)md)
      mexErrMsgIdAndTxt("mpcekf:arg", "max_steps: expected a non-negative integer");
    if (!(cd >= 1 && cd <= 2147483647.0) || cd != (double)(int32_t)cd)
      mexErrMsgIdAndTxt("mpcekf:arg", "stepuntil: chunk = %g is not a positive integer", cd);
    tmmax = (int32_t)md;
    tmchunk = (int32_t)cd;
    if (nrhs > 4 && !mxIsEmpty(prhs[4]) && (!mxIsDouble(prhs[4]) || mxIsComplex(prhs[4])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepuntil: tc: expected [] or ncells real doubles");
  }
  /* the balance commands likewise: output count, params that are no real doubles, a compensate
     that is not 0 / 1, an nsteps that is no non-negative integer, a tc of the wrong class */
  const int blbegin = !strcmp(cmd, "balancebegin"), stepbl = !strcmp(cmd, "stepexbalance");
  int32_t blcomp = 0, blsteps = 0;
  if ((blbegin || !strcmp(cmd, "balanceend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "balanceget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "balanceget: at most 1 output");
  if (stepbl && g_nlhs > 9)
    mexErrMsgIdAndTxt("mpcekf:arg",
                      "stepexbalance: at most 9 outputs [u, v, soc, phise, nexec, ucmd, limiter, bleed, zmin]");
  if (blbegin) {
    need(nrhs, 4, "'balancebegin', h, params, compensate");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "balancebegin: params: expected ncells x 3 real doubles");
    const double cd = scalar(prhs[3], "balancebegin: compensate");
    if (cd != 0.0 && cd != 1.0) mexErrMsgIdAndTxt("mpcekf:arg", "balancebegin: compensate = %g is not 0 or 1", cd);
    blcomp = (int32_t)cd;
  }
  if (stepbl) {
    need(nrhs, 3, "'stepexbalance', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    blsteps = (int32_t)nsd;
    if (nrhs > 3 && !mxIsEmpty(prhs[3]) && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepexbalance: tc: expected [] or ncells x nsteps real doubles");
  }
  /* the charger commands likewise: output count, params that are no real doubles, an nsteps that
     is no non-negative integer, a tc of the wrong class */
  const int chbegin = !strcmp(cmd, "chargerbegin"), stepch = !strcmp(cmd, "stepexcharger");
  int32_t chsteps = 0;
  if ((chbegin || !strcmp(cmd, "chargerend")) && g_nlhs > 0) mexErrMsgIdAndTxt("mpcekf:arg", "%s: no output", cmd);
  if (!strcmp(cmd, "chargerget") && g_nlhs > 1) mexErrMsgIdAndTxt("mpcekf:arg", "chargerget: at most 1 output");
  if (stepch && g_nlhs > 9)
    mexErrMsgIdAndTxt("mpcekf:arg",
                      "stepexcharger: at most 9 outputs [u, v, soc, phise, nexec, ucmd, limiter, bal, chg]");
  if (chbegin) {
    need(nrhs, 3, "'chargerbegin', h, params");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]))
      mexErrMsgIdAndTxt("mpcekf:arg", "chargerbegin: params: expected nstrings x 2 real doubles");
  }
  if (stepch) {
    need(nrhs, 3, "'stepexcharger', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    chsteps = (int32_t)nsd;
    if (nrhs > 3 && !mxIsEmpty(prhs[3]) && (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])))
      mexErrMsgIdAndTxt("mpcekf:arg", "stepexcharger: tc: expected [] or ncells x nsteps real doubles");
  }
  mpcekf_ctx *h = handle(prhs[1]);
  int64_t n = 0;
  int32_t NM = 0, nz = 0, ncon = 0;
  chk(mpcekf_ctx_info(h, &n, &NM, &nz, &ncon));
  const size_t nc = (size_t)n, nzz = (size_t)nz + 2;
  if (!strcmp(cmd, "destroy")) {
    track(h, 0);
    chk(mpcekf_ctx_destroy(h));
  } else if (!strcmp(cmd, "init")) {
    need(nrhs, 4, "'init', h, soc0_pct, tc_degC");
    chk(mpcekf_init_cells(h, dvec(prhs[2], nc, "soc0"), dvec(prhs[3], nc, "tc")));
  } else if (!strcmp(cmd, "step")) {
    need(nrhs, 3, "'step', h, nsteps[, tc]");
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    const int32_t ns = (int32_t)nsd;
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)ns, "tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 4; ++i) plhs[i] = dmat(nc, (size_t)ns);
    plhs[4] = imat(nc, (size_t)ns);
    chk(mpcekf_step(h, ns, tc, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]), mxGetDoubles(plhs[2]),
                    mxGetDoubles(plhs[3]), (int32_t *)mxGetData(plhs[4]), 0));
  } else if (stepobs) {
    /* 'step' plus rows idx of the plant's observable record at every step (the state each
       step's OB_step starts from): ncells x numel(idx) x nsteps, the library's
       [nsteps][nslots][ncells] as it stands */
    const double nsd = scalar(prhs[2], "nsteps");
    if (!(nsd >= 0 && nsd <= 2147483647.0) || nsd != (double)(int32_t)nsd)
      mexErrMsgIdAndTxt("mpcekf:arg", "nsteps: expected a non-negative integer");
    const int32_t ns = (int32_t)nsd;
    int32_t off[MPCEKF_OBS_COUNT + 1];
    chk(mpcekf_obs_layout(h, off));
    const size_t k = mxGetNumberOfElements(prhs[3]);
    const double *idx = mxGetDoubles(prhs[3]); /* class, count and >= 1 checked above */
    int32_t *slots = (int32_t *)mxMalloc(k * sizeof(int32_t));
    for (size_t j = 0; j < k; ++j) {
      if (idx[j] > (double)off[MPCEKF_OBS_COUNT])
        mexErrMsgIdAndTxt("mpcekf:arg", "stepobs: idx(%zu) = %g is not a slot 1..%d", j + 1, idx[j],
                          (int)off[MPCEKF_OBS_COUNT]);
      slots[j] = (int32_t)idx[j] - 1;
    }
    const double *tc = nrhs > 4 ? opt_vec(prhs[4], nc * (size_t)ns, "tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 4; ++i) plhs[i] = dmat(nc, (size_t)ns);
    plhs[4] = imat(nc, (size_t)ns);
    const mwSize od[3] = {(mwSize)nc, (mwSize)k, (mwSize)ns};
    plhs[5] = dnd(3, od);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    chk(mpcekf_step_ex_obs(h, ns, tc, &tr, slots, (int32_t)k, mxGetDoubles(plhs[5]), 0));
    mxFree(slots);
  } else if (!strcmp(cmd, "plant")) {
    need(nrhs, 3, "'plant', h, iapp[, tc]");
    plhs[0] = dmat(1, nc);
    chk(mpcekf_plant_step(h, dvec(prhs[2], nc, "iapp"), nrhs > 3 ? opt_vec(prhs[3], nc, "tc") : NULL,
                          mxGetDoubles(plhs[0])));
  } else if (!strcmp(cmd, "plantobs")) {
    need(nrhs, 3, "'plantobs', h, iapp[, tc]");
    static const char *const obs_names[MPCEKF_OBS_COUNT] = {
        "negSOC", "posSOC", "cellSOC", "negIfdl", "posIfdl", "negIfdl0", "posIfdl3", "negIf", "posIf",
        "negIf0", "posIf3", "negIdl", "posIdl", "negThetass", "posThetass", "negThetass0", "posThetass3",
        "negPhise", "posPhise", "negPhise0", "Phie", "Thetae", "negPhis", "posPhis", "Vcell"};
    int32_t off[MPCEKF_OBS_COUNT + 1];
    chk(mpcekf_obs_layout(h, off));
    const double *iapp = dvec(prhs[2], nc, "iapp"), *tc = nrhs > 3 ? opt_vec(prhs[3], nc, "tc") : NULL;
    const size_t nobs = (size_t)off[MPCEKF_OBS_COUNT];
    plhs[0] = dmat(1, nc);
    if (g_nlhs < 2) { /* v = plantobs(..): the record stays on the device for 'obsslots' */
      chk(mpcekf_plant_step_obs(h, iapp, tc, mxGetDoubles(plhs[0]), NULL));
      return;
    }
    /* the record is slot-major [nobs][ncells]; a field is len x ncells column-major */
    double *rec = (double *)mxMalloc(nobs * nc * sizeof(double) + 8);
    chk(mpcekf_plant_step_obs(h, iapp, tc, mxGetDoubles(plhs[0]), rec));
    plhs[1] = mxCreateStructMatrix(1, 1, MPCEKF_OBS_COUNT, (const char **)obs_names);
    for (int f = 0; f < MPCEKF_OBS_COUNT; ++f) {
      const size_t len = (size_t)(off[f + 1] - off[f]);
      mxArray *a = dmat(len, nc);
      double *d = mxGetDoubles(a);
      for (size_t i = 0; i < len; ++i)
        for (size_t c = 0; c < nc; ++c) d[i + len * c] = rec[((size_t)off[f] + i) * nc + c];
      mxSetField(plhs[1], 0, obs_names[f], a);
    }
    mxFree(rec);
  } else if (!strcmp(cmd, "obslayout")) {
    /* off = mpcekf_mex('obslayout', h): 1 x 26 doubles, field f (the order of 'plantobs') is
       slots off(f)+1 .. off(f+1) of the record, off(end) = nobs */
    int32_t off[MPCEKF_OBS_COUNT + 1];
    chk(mpcekf_obs_layout(h, off));
    plhs[0] = dmat(1, MPCEKF_OBS_COUNT + 1);
    for (int f = 0; f <= MPCEKF_OBS_COUNT; ++f) mxGetDoubles(plhs[0])[f] = (double)off[f];
  } else if (!strcmp(cmd, "obsslots")) {
    int32_t off[MPCEKF_OBS_COUNT + 1];
    chk(mpcekf_obs_layout(h, off));
    const size_t k = mxGetNumberOfElements(prhs[2]);
    const double *idx = mxGetDoubles(prhs[2]); /* class, count and >= 1 checked above */
    int32_t *slots = (int32_t *)mxMalloc(k * sizeof(int32_t));
    for (size_t j = 0; j < k; ++j) {
      if (idx[j] > (double)off[MPCEKF_OBS_COUNT])
        mexErrMsgIdAndTxt("mpcekf:arg", "obsslots: idx(%zu) = %g is not a slot 1..%d", j + 1, idx[j],
                          (int)off[MPCEKF_OBS_COUNT]);
      slots[j] = (int32_t)idx[j] - 1;
    }
    double *rows = (double *)mxMalloc(k * nc * sizeof(double) + 8); /* [k][ncells] */
    chk(mpcekf_plant_obs_slots(h, slots, (int32_t)k, rows));
    plhs[0] = dmat(k, nc);
    for (size_t j = 0; j < k; ++j)
      for (size_t c = 0; c < nc; ++c) mxGetDoubles(plhs[0])[j + k * c] = rows[j * nc + c];
    mxFree(rows);
    mxFree(slots);
  } else if (!strcmp(cmd, "ekf")) {
    need(nrhs, 4, "'ekf', h, vk, ik[, tk]");
    /* [zk, zbk, xm, xg]: Xind crosses back only when asked for (nargout > 2); it stays on
       the device for 'linearize' with empty zk / xm / xg either way */
    const int want_x = g_nlhs > 2;
    plhs[0] = dmat(nzz, nc);
    plhs[1] = dmat(nzz, nc);
    plhs[2] = want_x ? imat(4, nc) : mxCreateDoubleMatrix(0, 0, mxREAL);
    plhs[3] = want_x ? dmat(4, nc) : mxCreateDoubleMatrix(0, 0, mxREAL);
    chk(mpcekf_ekf_step(h, dvec(prhs[2], nc, "vk"), dvec(prhs[3], nc, "ik"),
                        nrhs > 4 ? opt_vec(prhs[4], nc, "tk") : NULL, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]),
                        want_x ? (int32_t *)mxGetData(plhs[2]) : NULL, want_x ? mxGetDoubles(plhs[3]) : NULL));
  } else if (!strcmp(cmd, "linearize")) {
    need(nrhs, 5, "'linearize', h, zk, xm, xg[, tk]");
    /* empty zk, xm, xg: the device copies of the last 'ekf'; the records stay on the device
       (plhs[0] empty) for 'mpc' / 'mpcdiag' with an empty lin and for 'linfields' */
    const double *tk = nrhs > 5 ? opt_vec(prhs[5], nc, "tk") : NULL;
    if (mxIsEmpty(prhs[2]) && mxIsEmpty(prhs[3]) && mxIsEmpty(prhs[4])) {
      plhs[0] = mxCreateDoubleMatrix(0, 0, mxREAL);
      chk(mpcekf_linearize(h, NULL, NULL, NULL, tk, NULL));
    } else {
      plhs[0] = dmat(MPCEKF_LIN_SIZE, nc);
      chk(mpcekf_linearize(h, dvec(prhs[2], nzz * nc, "zk"), ivec(prhs[3], 4 * nc, "xm (4 x ncells)"),
                           dvec(prhs[4], 4 * nc, "xg"), tk, mxGetDoubles(plhs[0])));
    }
  } else if (!strcmp(cmd, "mpc")) {
    need(nrhs, 4, "'mpc', h, lin, soc_k1");
    /* [uk, nexec, J_uncon, J_final, norm_DU, viol]: iterMPC.m's command and its
       mpcData.cost row (iterMPC.m:89-95), 1 x ncells each */
    for (int i = 0; i < 6; ++i) plhs[i] = (i == 1 || i == 5) ? imat(1, nc) : dmat(1, nc);
    chk(mpcekf_mpc_step_ex(h, opt_vec(prhs[2], MPCEKF_LIN_SIZE * nc, "lin"), dvec(prhs[3], nc, "soc_k1"),
                           mxGetDoubles(plhs[0]), (int32_t *)mxGetData(plhs[1]), mxGetDoubles(plhs[2]),
                           mxGetDoubles(plhs[3]), mxGetDoubles(plhs[4]), (int32_t *)mxGetData(plhs[5])));
  } else if (!strcmp(cmd, "graph")) {
    if (nrhs < 3) mexErrMsgIdAndTxt("mpcekf:arg", "graph: enable flag");
    chk(mpcekf_set_graph(h, (int32_t)(mxGetScalar(prhs[2]) != 0.0)));
  } else if (setlim) {
    /* ncells x numel(idx) column-major is the library's [nfields][ncells] as it stands */
    chk(mpcekf_set_limits(h, (int32_t)nlimf, limf, dvec(prhs[3], nc * nlimf, "setlimits: values (ncells x numel(idx))")));
  } else if (getlim) {
    plhs[0] = dmat(nc, nlimf);
    chk(mpcekf_get_limits(h, (int32_t)nlimf, limf, mxGetDoubles(plhs[0])));
  } else if (!strcmp(cmd, "clearlimits")) {
    chk(mpcekf_clear_limits(h));
  } else if (sumbegin) {
    int32_t off[MPCEKF_OBS_COUNT + 1];
    chk(mpcekf_obs_layout(h, off));
    if (sumslot >= off[MPCEKF_OBS_COUNT])
      mexErrMsgIdAndTxt("mpcekf:arg", "summarybegin: slot = %d is not a slot 1..%d (0 or []: none)", (int)sumslot + 1,
                        (int)off[MPCEKF_OBS_COUNT]);
    chk(mpcekf_summary_begin(h, nrhs > 2 ? opt_vec(prhs[2], nc, "summarybegin: reach (ncells)") : NULL, sumslot));
  } else if (stepsum) {
    chk(mpcekf_step_summary(h, sumsteps, nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)sumsteps, "tc (ncells x nsteps)") : NULL));
  } else if (!strcmp(cmd, "getsummary")) {
    static const char *const sum_names[MPCEKF_NSUM] = {
        "seen", "steps", "err_step", "t_reach", "u_min", "u_min_step", "u_max", "v_max", "v_max_step", "v_min",
        "phise_min", "phise_min_step", "u_last", "v_last", "soc_last", "phise_last", "u_sum", "nexec_sum",
        "nexec_max", "nsat", "obs_min", "obs_min_step", "obs_max", "obs_max_step"};
    mxArray *a[MPCEKF_NSUM];
    int32_t ids[MPCEKF_NSUM];
    /* [nfields][ncells]: one scratch block, then a column vector per field */
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NSUM * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NSUM; ++f) ids[f] = f;
    chk(mpcekf_get_summary(h, MPCEKF_NSUM, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NSUM, (const char **)sum_names);
    for (int f = 0; f < MPCEKF_NSUM; ++f) {
      a[f] = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a[f]), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, sum_names[f], a[f]);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "summaryend")) {
    chk(mpcekf_summary_end(h));
  } else if (thbegin) {
    /* ncells x 3 column-major is the library's [MPCEKF_NTH][ncells] as it stands */
    chk(mpcekf_thermal_begin(h, dvec(prhs[2], nc * MPCEKF_NTH, "thermalbegin: params (ncells x 3)"),
                             (int32_t)mxGetNumberOfElements(prhs[3]), mxGetDoubles(prhs[3]),
                             nrhs > 4 ? opt_vec(prhs[4], nc, "thermalbegin: t0 (ncells)") : NULL));
  } else if (!strcmp(cmd, "thermalget")) {
    static const char *const th_names[MPCEKF_NTHR] = {"T", "T_max", "T_max_step", "T_min", "heat_sum", "steps", "nheld"};
    int32_t ids[MPCEKF_NTHR];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NTHR * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NTHR; ++f) ids[f] = f;
    chk(mpcekf_thermal_get(h, MPCEKF_NTHR, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NTHR, (const char **)th_names);
    for (int f = 0; f < MPCEKF_NTHR; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, th_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "thermalend")) {
    chk(mpcekf_thermal_end(h));
    /* a map with a temperature axis ended with the model: a refused one-field get changes nothing */
    int32_t id0 = 0;
    double *probe = (double *)mxMalloc(nc * sizeof(double) + 8);
    if (mpcekf_limit_map_get(h, 1, &id0, probe) != MPCEKF_OK) *mapnf_of(h) = 0;
    mxFree(probe);
  } else if (stepth) {
    for (int i = 0; i < 7; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)thsteps) : dmat(nc, (size_t)thsteps);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    chk(mpcekf_step_ex_thermal(h, thsteps, &tr, NULL, 0, NULL, mxGetDoubles(plhs[5]), mxGetDoubles(plhs[6]), 0));
  } else if (thsched) {
    /* ntab x numel(idx) x nsets column-major is the library's [nsets][nfields][ntab] as it stands */
    int32_t *set = NULL;
    if (nrhs > 6 && !mxIsEmpty(prhs[6])) {
      const double *sd = dvec(prhs[6], nc, "thermalschedule: sets (ncells)");
      set = (int32_t *)mxMalloc(nc * sizeof(int32_t) + 8);
      for (size_t c = 0; c < nc; ++c) set[c] = (int32_t)sd[c] - 1;
    }
    const int rc = mpcekf_thermal_schedule(h, (int32_t)nschf, schf, (int32_t)schtab, sch_lo, sch_hi, (int32_t)schsets,
                                           mxGetDoubles(prhs[5]), set);
    if (set) mxFree(set);
    chk(rc);
  } else if (!strcmp(cmd, "thermalscheduleend")) {
    chk(mpcekf_thermal_schedule_end(h));
  } else if (lmset) {
    /* nz x nt x numel(idx) x nsets column-major is the library's [nsets][nfields][nt][nz] as it stands */
    int32_t *set = NULL;
    if (nrhs > 9 && !mxIsEmpty(prhs[9])) {
      const double *sd = dvec(prhs[9], nc, "limitmap: sets (ncells)");
      set = (int32_t *)mxMalloc(nc * sizeof(int32_t) + 8);
      for (size_t c = 0; c < nc; ++c) set[c] = (int32_t)sd[c] - 1;
    }
    const double *z0 = nrhs > 10 ? opt_vec(prhs[10], nc, "limitmap: z0 (ncells)") : NULL;
    const int rc = mpcekf_limit_map(h, (int32_t)nlmf, lmf, (int32_t)lmnz, lm_zlo, lm_zhi, (int32_t)lmnt, lm_tlo, lm_thi,
                                    lminterp, (int32_t)lmsets, mxGetDoubles(prhs[7]), set, z0);
    if (set) mxFree(set);
    chk(rc);
    *mapnf_of(h) = (int32_t)nlmf;
  } else if (!strcmp(cmd, "limitmapget")) {
    static const char *const lm_names[MPCEKF_NLM] = {"z_last", "neval", "nclamp_z", "nclamp_t"};
    int32_t ids[MPCEKF_NLM];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NLM * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NLM; ++f) ids[f] = f;
    chk(mpcekf_limit_map_get(h, MPCEKF_NLM, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NLM, (const char **)lm_names);
    for (int f = 0; f < MPCEKF_NLM; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, lm_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "limitmapend")) {
    chk(mpcekf_limit_map_end(h));
    *mapnf_of(h) = 0;
  } else if (steplm) {
    /* without a 'limitmap' the library refuses the call before it touches a row; lim is
       ncells x (numel(idx) * nsteps): column (j, t) = field idx(j) at step t */
    const size_t nf = (size_t)*mapnf_of(h);
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)lmsteps, "stepexmap: tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 5; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)lmsteps) : dmat(nc, (size_t)lmsteps);
    plhs[5] = dmat(nc, (nf ? nf : 1) * (size_t)lmsteps);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    chk(mpcekf_step_ex_map(h, lmsteps, tc, &tr, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
                           mxGetDoubles(plhs[5]), 0));
  } else if (tcset) {
    chk(mpcekf_thermal_couple(h, dvec(prhs[2], nc, "thermalcouple: r_link (ncells)")));
  } else if (!strcmp(cmd, "thermalcoupleget")) {
    static const char *const tc_names[MPCEKF_NTCR] = {"nb_sum", "dt_max", "dt_max_step"};
    int32_t ids[MPCEKF_NTCR];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NTCR * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NTCR; ++f) ids[f] = f;
    chk(mpcekf_thermal_couple_get(h, MPCEKF_NTCR, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NTCR, (const char **)tc_names);
    for (int f = 0; f < MPCEKF_NTCR; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, tc_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "thermalcoupleend")) {
    chk(mpcekf_thermal_couple_end(h));
  } else if (steptc) {
    for (int i = 0; i < 8; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)tcsteps) : dmat(nc, (size_t)tcsteps);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    chk(mpcekf_step_ex_couple(h, tcsteps, NULL, &tr, NULL, 0, NULL, mxGetDoubles(plhs[5]), mxGetDoubles(plhs[6]), NULL,
                              NULL, NULL, mxGetDoubles(plhs[7]), 0));
  } else if (pkbegin) {
    chk(mpcekf_pack_begin(h, pkseries));
    *series_of(h) = pkseries;
  } else if (!strcmp(cmd, "packget")) {
    static const char *const pk_names[MPCEKF_NPK] = {"nlim", "steps", "headroom"};
    int32_t ids[MPCEKF_NPK];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NPK * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NPK; ++f) ids[f] = f;
    chk(mpcekf_pack_get(h, MPCEKF_NPK, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NPK, (const char **)pk_names);
    for (int f = 0; f < MPCEKF_NPK; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, pk_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "packend")) {
    chk(mpcekf_pack_end(h));
    *series_of(h) = 0;
  } else if (steppk) {
    /* without a 'packbegin' the library refuses the call before it touches a row */
    const int32_t series = *series_of(h);
    const size_t nstr = series ? nc / (size_t)series : 0;
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)pksteps, "stepexpack: tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 6; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)pksteps) : dmat(nc, (size_t)pksteps);
    plhs[6] = imat(nstr, (size_t)pksteps);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    int32_t *lim = (int32_t *)mxGetData(plhs[6]);
    chk(mpcekf_step_ex_pack(h, pksteps, tc, &tr, NULL, 0, NULL, NULL, NULL, mxGetDoubles(plhs[5]), series ? lim : NULL, 0));
    for (size_t i = 0; i < nstr * (size_t)pksteps; ++i) lim[i] += 1; /* 1-based; 0: no command */
  } else if (blbegin) {
    /* ncells x 3 column-major is the library's [MPCEKF_NBLP][ncells] as it stands */
    chk(mpcekf_balance_begin(h, dvec(prhs[2], nc * MPCEKF_NBLP, "balancebegin: params (ncells x 3)"), blcomp));
  } else if (!strcmp(cmd, "balanceget")) {
    static const char *const bl_names[MPCEKF_NBL] = {"steps_on", "q_bleed", "switches", "dz_max", "dz_last", "steps"};
    int32_t ids[MPCEKF_NBL];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NBL * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NBL; ++f) ids[f] = f;
    chk(mpcekf_balance_get(h, MPCEKF_NBL, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NBL, (const char **)bl_names);
    for (int f = 0; f < MPCEKF_NBL; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, bl_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "balanceend")) {
    chk(mpcekf_balance_end(h));
  } else if (stepbl) {
    /* without a 'balancebegin' the library refuses the call before it touches a row */
    const int32_t series = *series_of(h);
    const size_t nstr = series ? nc / (size_t)series : 0;
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)blsteps, "stepexbalance: tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 6; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)blsteps) : dmat(nc, (size_t)blsteps);
    plhs[6] = imat(nstr, (size_t)blsteps);
    plhs[7] = dmat(nc, (size_t)blsteps);
    plhs[8] = dmat(nstr, (size_t)blsteps);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    int32_t *lim = (int32_t *)mxGetData(plhs[6]);
    chk(mpcekf_step_ex_balance(h, blsteps, tc, &tr, NULL, 0, NULL, NULL, NULL, mxGetDoubles(plhs[5]),
                               series ? lim : NULL, mxGetDoubles(plhs[7]), series ? mxGetDoubles(plhs[8]) : NULL, 0));
    for (size_t i = 0; i < nstr * (size_t)blsteps; ++i) lim[i] += 1; /* 1-based; 0: no command */
  } else if (chbegin) {
    /* nstrings x 2 column-major is the library's [MPCEKF_NCHP][nstrings] as it stands; without a
       'packbegin' the library refuses the call whatever the size */
    const int32_t series = *series_of(h);
    const size_t nstr = series ? nc / (size_t)series : nc;
    chk(mpcekf_charger_begin(h, dvec(prhs[2], nstr * MPCEKF_NCHP, "chargerbegin: params (nstrings x 2)")));
  } else if (!strcmp(cmd, "chargerget")) {
    static const char *const ch_names[MPCEKF_NCH] = {"steps", "ncap_i", "ncap_p", "q", "e", "curtail",
                                                     "p_min", "v_peak", "nvalid_min"};
    const int32_t series = *series_of(h);
    const size_t nstr = series ? nc / (size_t)series : nc;
    int32_t ids[MPCEKF_NCH];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NCH * nstr * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NCH; ++f) ids[f] = f;
    chk(mpcekf_charger_get(h, MPCEKF_NCH, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NCH, (const char **)ch_names);
    for (int f = 0; f < MPCEKF_NCH; ++f) {
      mxArray *a = dmat(nstr, 1);
      if (nstr) memcpy(mxGetDoubles(a), vals + (size_t)f * nstr, nstr * sizeof(double));
      mxSetField(plhs[0], 0, ch_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "chargerend")) {
    chk(mpcekf_charger_end(h));
  } else if (stepch) {
    /* without a 'chargerbegin' the library refuses the call before it touches a row */
    static const char *const bal_names[2] = {"bleed", "zmin"};
    static const char *const chg_names[3] = {"vstr", "istr", "capby"};
    const int32_t series = *series_of(h);
    const size_t nstr = series ? nc / (size_t)series : 0;
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)chsteps, "stepexcharger: tc (ncells x nsteps)") : NULL;
    /* a balancer's rows only where there is one: a refused one-field get changes nothing */
    int32_t id0 = 0;
    double *probe = (double *)mxMalloc(nc * sizeof(double) + 8);
    const int has_bal = mpcekf_balance_get(h, 1, &id0, probe) == MPCEKF_OK;
    mxFree(probe);
    for (int i = 0; i < 6; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)chsteps) : dmat(nc, (size_t)chsteps);
    plhs[6] = imat(nstr, (size_t)chsteps);
    mxArray *bleed = has_bal ? dmat(nc, (size_t)chsteps) : dmat(0, 0);
    mxArray *zmin = has_bal ? dmat(nstr, (size_t)chsteps) : dmat(0, 0);
    mxArray *vstr = dmat(nstr, (size_t)chsteps), *istr = dmat(nstr, (size_t)chsteps), *capby = imat(nstr, (size_t)chsteps);
    plhs[7] = mxCreateStructMatrix(1, 1, 2, (const char **)bal_names);
    mxSetField(plhs[7], 0, "bleed", bleed);
    mxSetField(plhs[7], 0, "zmin", zmin);
    plhs[8] = mxCreateStructMatrix(1, 1, 3, (const char **)chg_names);
    mxSetField(plhs[8], 0, "vstr", vstr);
    mxSetField(plhs[8], 0, "istr", istr);
    mxSetField(plhs[8], 0, "capby", capby);
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    int32_t *lim = (int32_t *)mxGetData(plhs[6]);
    chk(mpcekf_step_ex_charger(h, chsteps, tc, &tr, NULL, 0, NULL, NULL, NULL, mxGetDoubles(plhs[5]), series ? lim : NULL,
                               has_bal ? mxGetDoubles(bleed) : NULL, has_bal && series ? mxGetDoubles(zmin) : NULL,
                               series ? mxGetDoubles(vstr) : NULL, series ? mxGetDoubles(istr) : NULL,
                               series ? (int32_t *)mxGetData(capby) : NULL, 0));
    for (size_t i = 0; i < nstr * (size_t)chsteps; ++i) lim[i] += 1; /* 1-based; 0: no command, -1: capped */
  } else if (tmbegin) {
    /* ncells x 3 column-major is the library's [MPCEKF_NTMP][ncells] as it stands */
    chk(mpcekf_term_begin(h, dvec(prhs[2], nc * MPCEKF_NTMP, "termbegin: params (ncells x 3)"), tmhold));
  } else if (!strcmp(cmd, "termget")) {
    static const char *const tm_names[MPCEKF_NTM] = {"state", "done_step", "reason", "soc_done",
                                                     "u_done", "T_done", "rest", "steps"};
    int32_t ids[MPCEKF_NTM];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NTM * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NTM; ++f) ids[f] = f;
    chk(mpcekf_term_get(h, MPCEKF_NTM, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NTM, (const char **)tm_names);
    for (int f = 0; f < MPCEKF_NTM; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, tm_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "termend")) {
    chk(mpcekf_term_end(h));
  } else if (until) {
    const double *tc = nrhs > 4 ? opt_vec(prhs[4], nc, "stepuntil: tc (ncells)") : NULL;
    int32_t run = 0;
    int64_t left = 0;
    chk(mpcekf_step_until(h, tmmax, tmchunk, tc, &run, &left));
    plhs[0] = mxCreateDoubleScalar((double)run);
    plhs[1] = mxCreateDoubleScalar((double)left);
  } else if (agbegin) {
    /* ncells x 5 x nreact column-major is the library's [nreact][MPCEKF_NAGP][ncells] as it stands */
    chk(mpcekf_aging_begin(h, agreact, agsrc, dvec(prhs[2], nc * MPCEKF_NAGP * (size_t)agreact, "agingbegin: params (ncells x 5 x nreact)")));
    *agrows_of(h) = ((agsrc & 1) + (agsrc >> 1)) * agreact;
  } else if (agget) {
    static const char *const ag_names[MPCEKF_NAGR] = {"q_sum", "j_max", "j_max_step", "n_on", "steps", "nskip"};
    int32_t ids[MPCEKF_NAGR];
    double *vals = (double *)mxMalloc((size_t)MPCEKF_NAGR * nc * sizeof(double) + 8);
    for (int f = 0; f < MPCEKF_NAGR; ++f) ids[f] = f;
    chk(mpcekf_aging_get(h, agsrc, agreact, MPCEKF_NAGR, ids, vals));
    plhs[0] = mxCreateStructMatrix(1, 1, MPCEKF_NAGR, (const char **)ag_names);
    for (int f = 0; f < MPCEKF_NAGR; ++f) {
      mxArray *a = dmat(nc, 1);
      if (nc) memcpy(mxGetDoubles(a), vals + (size_t)f * nc, nc * sizeof(double));
      mxSetField(plhs[0], 0, ag_names[f], a);
    }
    mxFree(vals);
  } else if (!strcmp(cmd, "agingend")) {
    chk(mpcekf_aging_end(h));
    *agrows_of(h) = 0;
  } else if (stepag) {
    /* without an 'agingbegin' the library refuses the call before it touches a row */
    const size_t rows = (size_t)*agrows_of(h);
    const double *tc = nrhs > 3 ? opt_vec(prhs[3], nc * (size_t)agsteps, "stepexaging: tc (ncells x nsteps)") : NULL;
    for (int i = 0; i < 5; ++i) plhs[i] = i == 4 ? imat(nc, (size_t)agsteps) : dmat(nc, (size_t)agsteps);
    plhs[5] = dmat(nc, rows * (size_t)agsteps); /* ncells x (nsrc*nreact) x nsteps, its pages side by side */
    mpcekf_traj tr;
    memset(&tr, 0, sizeof tr);
    tr.u = mxGetDoubles(plhs[0]); tr.v = mxGetDoubles(plhs[1]); tr.soc = mxGetDoubles(plhs[2]);
    tr.phise = mxGetDoubles(plhs[3]); tr.nexec = (int32_t *)mxGetData(plhs[4]);
    chk(mpcekf_step_ex_aging(h, agsteps, tc, &tr, NULL, 0, NULL, NULL, NULL, NULL, NULL, rows ? mxGetDoubles(plhs[5]) : NULL, 0));
  } else if (!strcmp(cmd, "mpcdiag")) {
    need(nrhs, 3, "'mpcdiag', h, lin[, uk_1]");
    plhs[0] = mxCreateDoubleMatrix(7, (mwSize)nc, mxCOMPLEX);  /* interleaved (re, im): [ncells][7][2] */
    plhs[1] = dmat(7, nc);
    chk(mpcekf_mpc_diag(h, opt_vec(prhs[2], MPCEKF_LIN_SIZE * nc, "lin"), nrhs > 3 ? opt_vec(prhs[3], nc, "uk_1") : NULL,
                        (double *)mxGetComplexDoubles(plhs[0]), mxGetDoubles(plhs[1])));
  } else if (!strcmp(cmd, "get_state") || !strcmp(cmd, "set_state")) {
    /* the model-blend EKF state (xhat, SigmaX 6 x 6) is part of an MB context's checkpoint */
    mpcekf_config cc;
    chk(mpcekf_ctx_config(h, &cc));
    const int nf = cc.method == MPCEKF_METHOD_MB ? 7 : 6;
    const char *f[] = {"bigX", "ekf", "scal", "lambda", "warn", "status", "mb"};
    const size_t rows[] = {(size_t)NM * 6, (size_t)NM * 20, MPCEKF_NSCAL, (size_t)ncon, 1, 1, MPCEKF_MB_SIZE};
    mpcekf_state st;
    memset(&st, 0, sizeof st);
    if (cmd[0] == 'g') {
      plhs[0] = mxCreateStructMatrix(1, 1, nf, f);
      mxArray *a[7];
      for (int i = 0; i < nf; ++i) {
        a[i] = (i == 4 || i == 5) ? imat(1, nc) : dmat(rows[i], nc);
        mxSetField(plhs[0], 0, f[i], a[i]);
      }
      st.bigX = mxGetDoubles(a[0]); st.ekf = mxGetDoubles(a[1]); st.scal = mxGetDoubles(a[2]);
      st.lambda = mxGetDoubles(a[3]); st.warn = (int32_t *)mxGetData(a[4]); st.status = (int32_t *)mxGetData(a[5]);
      if (nf == 7) st.mb = mxGetDoubles(a[6]);
      chk(mpcekf_get_state(h, &st));
    } else {
      if (nrhs < 3 || !mxIsStruct(prhs[2])) mexErrMsgIdAndTxt("mpcekf:arg", "set_state(h, st): st must be a struct");
      const mxArray *s = prhs[2];
      st.bigX = (double *)dvec(field(s, "bigX"), rows[0] * nc, "bigX");
      st.ekf = (double *)dvec(field(s, "ekf"), rows[1] * nc, "ekf");
      st.scal = (double *)dvec(field(s, "scal"), rows[2] * nc, "scal");
      st.lambda = (double *)dvec(field(s, "lambda"), rows[3] * nc, "lambda");
      st.warn = ivec(field(s, "warn"), nc, "warn");
      st.status = ivec(field(s, "status"), nc, "status");
      /* an MB checkpoint saved before st.mb existed restores without it (NULL keeps the
         context's blend state, as the C-ABI allows) */
      if (nf == 7 && mxGetField(s, 0, "mb")) st.mb = (double *)dvec(mxGetField(s, 0, "mb"), rows[6] * nc, "mb (MB context)");
      chk(mpcekf_set_state(h, &st));
    }
  } else if (!strcmp(cmd, "linfields")) {
    /* out = mpcekf_mex('linfields', h, idx[, set]): rows idx (1-based MPCEKF_LIN_* + 1) of
       the device-resident records of the last 'linearize' with empty zk, k x ncells; set
       (k x ncells) is written into them first */
    need(nrhs, 3, "'linfields', h, idx[, set]");
    const size_t k = mxGetNumberOfElements(prhs[2]);
    if (k < 1 || k > MPCEKF_LIN_SIZE) mexErrMsgIdAndTxt("mpcekf:arg", "linfields: 1..%d slot indices", MPCEKF_LIN_SIZE);
    const double *idx = dvec(prhs[2], k, "idx");
    int32_t slots[MPCEKF_LIN_SIZE];
    for (size_t j = 0; j < k; ++j) {
      if (!(idx[j] >= 1 && idx[j] <= MPCEKF_LIN_SIZE) || idx[j] != (double)(int)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "linfields: idx(%zu) = %g is not a slot 1..%d", j + 1, idx[j], MPCEKF_LIN_SIZE);
      slots[j] = (int32_t)idx[j] - 1;
    }
    plhs[0] = dmat(k, nc);
    chk(mpcekf_lin_fields(h, slots, (int32_t)k, nrhs > 3 ? opt_vec(prhs[3], k * nc, "set (k x ncells)") : NULL,
                          mxGetDoubles(plhs[0])));
  } else if (!strcmp(cmd, "scalars")) {
    need(nrhs, 3, "'scalars', h, idx");
    const size_t k = mxGetNumberOfElements(prhs[2]);
    if (k < 1 || k > MPCEKF_NSCAL) mexErrMsgIdAndTxt("mpcekf:arg", "scalars: 1..%d slot indices", MPCEKF_NSCAL);
    const double *idx = dvec(prhs[2], k, "idx");
    int32_t slots[MPCEKF_NSCAL];
    for (size_t j = 0; j < k; ++j) {
      if (!(idx[j] >= 1 && idx[j] <= MPCEKF_NSCAL) || idx[j] != (double)(int)idx[j])
        mexErrMsgIdAndTxt("mpcekf:arg", "scalars: idx(%zu) = %g is not a slot 1..%d", j + 1, idx[j], MPCEKF_NSCAL);
      slots[j] = (int32_t)idx[j] - 1;
    }
    plhs[0] = dmat(k, nc); /* k x ncells column-major = the library's [ncells][k] */
    plhs[1] = imat(1, nc);
    plhs[2] = imat(1, nc);
    chk(mpcekf_get_scalars(h, slots, (int32_t)k, mxGetDoubles(plhs[0]), (int32_t *)mxGetData(plhs[1]),
                           (int32_t *)mxGetData(plhs[2])));
  } else {
    mexErrMsgIdAndTxt("mpcekf:arg", "unknown command %s", cmd);
  }
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  mxArray *out[MAXOUT] = {0};
  g_nlhs = nlhs;
  gateway(out, nrhs, prhs);
  const int keep = nlhs < 1 ? 1 : nlhs;
  if (keep > MAXOUT) mexErrMsgIdAndTxt("mpcekf:arg", "too many outputs");
  for (int i = 0; i < MAXOUT; ++i) {
    if (i < keep) {
      if (i > 0 && !out[i]) mexErrMsgIdAndTxt("mpcekf:arg", "output %d is not defined for this command", i + 1);
      plhs[i] = out[i];
    } else if (out[i]) {
      mxDestroyArray(out[i]);
    }
  }
}
