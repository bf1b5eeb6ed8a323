// mpcekf_mpc_sw.inc -- the body of k_mpc_sw<SW> and k_mpc_pc<SW> (mpcekf_switch.hip), included in
// both after c, n and the bounds check: iterMPC.m:17-66 and, without a QP, :75-95 on the
// linearisation record, reading the limits from the KCfg named cf (the kernel argument in
// k_mpc_sw, the cell's own copy in k_mpc_pc).  One text, so the two kernels cannot drift apart, and
// k_mpc_sw's token stream is the one it had as a single kernel.
  const bool fused = io.mode & MODE_FUSED;
  s.hflag[c] = 0;  // set again only if hildreth.m must run
  if (s.status[c] & ST_ERROR) {  // the fused step's k_cell already wrote this cell's NaN outputs
    if (!fused) {
      const double NaN = __builtin_nan("");
      if (io.uk_out) io.uk_out[c] = NaN;
      if (io.nexec) io.nexec[c] = 0;
      if (io.junc_out) io.junc_out[c] = NaN;
      if (io.jfin_out) io.jfin_out[c] = NaN;
      if (io.normdu_out) io.normdu_out[c] = NaN;
      if (io.nviol_out) io.nviol_out[c] = 0;
    }
    return;
  }
  Lin L;
  lin_load(io.lin_in + c * 35, L);
  const double Zsoc = io.soc_k1_in[c];
  double uk_1 = s.uk_1[c];
  MpcOut o;
  MpcSetup Pm;
  const bool need = mpc_setup<NP, NC, SW>(cf, L, uk_1, Zsoc, Pm, o);
  if (s.J_unc) s.J_unc[c] = o.J_unc;
  if (io.junc_out) io.junc_out[c] = o.J_unc;
  s.hflag[c] = need ? 1 : 0;
  if (need) {  // hildreth.m runs in k_hild_sw; a disabled block's Hv / He / gamma fields are +0
    double *pb = s.prob;
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
    mpc_finish<NP, NC, SW>(Pm.Cn, Pm.e, Pm.Ru, Pm.DU, uk_1, o);
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
