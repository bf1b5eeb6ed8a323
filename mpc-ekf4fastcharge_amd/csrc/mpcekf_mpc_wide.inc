// mpcekf_mpc_wide.inc -- the body of k_mpc_wide and k_mpc_wide_pc (mpcekf_wide.hip), included in
// both after T, c, n and the bounds check: iterMPC.m:17-66 per cell (mpc_setup's arithmetic,
// streamed), reading the limits from the KCfg named cf (the kernel argument in k_mpc_wide, the
// cell's own copy in k_mpc_wide_pc).  One text for both; k_mpc_wide's token stream is unchanged.
  const bool fused = io.mode & MODE_FUSED;
  s.hflag[c] = 0;
  if (s.status[c] & ST_ERROR) {  // the fused step's iterEKF kernel already wrote NaN outputs
    if (!fused) {
      if (io.uk_out) io.uk_out[c] = __builtin_nan("");
      if (io.nexec) io.nexec[c] = 0;
    }
    return;
  }
  double *pb = w.prob;
  Lin L;
  lin_load(io.lin_in + c * 35, L);
  const double SOCk_1 = io.soc_k1_in[c];
  const double uk_1 = s.uk_1[c];
  double dx[NA];
#pragma unroll
  for (int k = 0; k < 6; ++k) dx[k] = L.xhat[k];
  dx[6] = uk_1;
  // predMat(Csoc): Hs, e = Ref - Phi_soc*dx (iterMPC.m:20-35); the SOC constraint rows'
  // gamma (constraintsMPC.m:89-101) from the same Phi_soc*dx
  double Hs[NP], e[NP], gs[NP];
  {
    double S[6], P[6], Cb[7], row[7];
#pragma unroll
    for (int j = 0; j < 6; ++j) { S[j] = 0.0; P[j] = 1.0; Cb[j] = L.Csoc[j]; }
    Cb[6] = L.Dsoc;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      pred_step(L.a, Cb, S, P, Hs[k], row);
      const double acc = rowdot(row, dx);
      e[k] = cf.ref * 1.0 - acc;
      gs[k] = cf.zmax * 1.0 - (acc + SOCk_1 * 1.0);
    }
  }
  double F[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) acc = acc + (-2 * (j <= i ? Hs[i - j] : 0.0)) * e[i];
    F[j] = acc;
  }
  // E = 2(G'G + Ru I), Ru = ||F|| / (2 du_max sqrt(Nc)) - sigma_min(G'G) (iterMPC.m:38-47).
  // G'G is formed twice (for the sigma_min cache test, then for E) rather than kept live.
  auto gtg = [&](int a, int b) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) acc = acc + (a <= i ? Hs[i - a] : 0.0) * (b <= i ? Hs[i - b] : 0.0);
    return acc;
  };
  bool hit = true;
#pragma unroll
  for (int a = 0; a < NC; ++a)
#pragma unroll
    for (int b = 0; b < NC; ++b) {
      const double gab = gtg(a, b);
      hit = hit && __double_as_longlong(gab) == __double_as_longlong(w.smin[a * NC + b]);
      pb[(T::E + a * NC + b) * n + c] = gab;
    }
  const double smin = hit ? w.smin[NC * NC] : sigma_min_cold<NC>(pb + T::E * n + c, n);
  double nF = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) nF = nF + F[j] * F[j];
  nF = sqrt(nF);
  const double Ru = (nF / (2 * cf.du_max * sqrt((double)NC))) - smin;
  double mE[NC][NC], DU[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    pb[(T::F + a) * n + c] = F[a];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
      const double eab = 2 * (gtg(a, b) + Ru * (a == b ? 1.0 : 0.0));
      pb[(T::E + a * NC + b) * n + c] = eab;
      mE[a][b] = -eab;
    }
  }
  lu_solve_n<NC>(mE, F, DU);  // DU = -E\F (iterMPC.m:48)
  const double J_unc = mpc_cost<NP, NC>(Hs, e, Ru, DU);
  if (s.J_unc) s.J_unc[c] = J_unc;
  if (io.junc_out) io.junc_out[c] = J_unc;
  // constraintsMPC.m rows: gamma to the record, M*DU - gamma tested as each row is formed
  int nv = 0, nviol = 0;
  // the row loops stay rolled (instruction fetch, see k_hild_prep); the G_v / -G_e rows'
  // M(k, :) is a shift register of the H column with mrow_vec's values
#pragma unroll 1
  for (int i = 0; i < 4 * NC; ++i) {
    const double g = i < NC ? (cf.u_max - uk_1) * 1.0 : i < 2 * NC ? -(cf.u_min - uk_1) * 1.0
                   : i < 3 * NC ? cf.du_max * 1.0 : -cf.du_min * 1.0;
    pb[(T::GAM + i) * n + c] = g;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NC; ++j) acc = acc + mconst<NC>(i, j) * DU[j];
    if (acc - g > 0) nv++;
    if (acc - g > 1e-9) nviol++;
  }
  {  // G_v rows: predMat(Cv, Dv), gamma = v_max - (Phi_v*dx + bv)
    double S[6], P[6], Cb[7], row[7], b[NC];
#pragma unroll
    for (int j = 0; j < 6; ++j) { S[j] = 0.0; P[j] = 1.0; Cb[j] = L.Cv[j]; }
    Cb[6] = L.Dv;
#pragma unroll
    for (int j = 0; j < NC; ++j) b[j] = 0.0;
#pragma unroll 1
    for (int k = 0; k < NP; ++k) {
      double Hvk;
      pred_step(L.a, Cb, S, P, Hvk, row);
      const double g = cf.v_max - (rowdot(row, dx) + L.bv * 1.0);
      pb[(T::GAM + 4 * NC + k) * n + c] = g;
      pb[(T::HV + k) * n + c] = Hvk;
#pragma unroll
      for (int j = NC - 1; j > 0; --j) b[j] = b[j - 1];
      b[0] = Hvk;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NC; ++j) acc = acc + b[j] * DU[j];
      if (acc - g > 0) nv++;
      if (acc - g > 1e-9) nviol++;
    }
  }
  {  // -G_e rows: predMat(Cphi, Dphi), gamma = -phise_min + (Phi_e*dx + bphi)
    double S[6], P[6], Cb[7], row[7], b[NC];
#pragma unroll
    for (int j = 0; j < 6; ++j) { S[j] = 0.0; P[j] = 1.0; Cb[j] = L.Cphi[j]; }
    Cb[6] = L.Dphi;
#pragma unroll
    for (int j = 0; j < NC; ++j) b[j] = -0.0;
#pragma unroll 1
    for (int k = 0; k < NP; ++k) {
      double Hek;
      pred_step(L.a, Cb, S, P, Hek, row);
      const double g = -cf.phise_min + (rowdot(row, dx) + L.bphi * 1.0);
      pb[(T::GAM + 4 * NC + NP + k) * n + c] = g;
      pb[(T::HE + k) * n + c] = Hek;
#pragma unroll
      for (int j = NC - 1; j > 0; --j) b[j] = b[j - 1];
      b[0] = -Hek;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NC; ++j) acc = acc + b[j] * DU[j];
      if (acc - g > 0) nv++;
      if (acc - g > 1e-9) nviol++;
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) {  // G_soc rows
    const double g = gs[k];
    pb[(T::GAM + 4 * NC + 2 * NP + k) * n + c] = g;
    pb[(T::HS + k) * n + c] = Hs[k];
    pb[(T::ERR + k) * n + c] = e[k];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NC; ++j) acc = acc + (j <= k ? Hs[k - j] : 0.0) * DU[j];
    if (acc - g > 0) nv++;
    if (acc - g > 1e-9) nviol++;
  }
  pb[T::RU * n + c] = Ru;
  pb[T::UK1 * n + c] = uk_1;
  if (nv == 0) {  // iterMPC.m:66-95 without hildreth.m: J_fin = J_unc (same DU)
    const double uk = DU[0] + uk_1;
    s.uk_1[c] = uk;
    if (s.J_fin) { s.J_fin[c] = J_unc; s.nviol[c] = nviol; }
    cost_out(io, c, J_unc, nviol, norm_du<NC>(DU));
    if (io.uk_out) io.uk_out[c] = uk;
    if (io.nexec) io.nexec[c] = 0;
    if (fused) {
      s.uk[c] = uk;
      if (io.u) io.u[c] = uk;
    }
    return;
  }
  s.hflag[c] = 1;
