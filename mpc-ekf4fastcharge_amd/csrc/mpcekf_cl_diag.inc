// mpcekf_cl_diag.inc -- the body of k_cl_diag and k_cl_diag_pc (mpcekf_mpc.hpp), included in both
// after c and the bounds check: iterMPC.m:53-60's poles / sv of one cell, reading the limits
// (du_max in Ru, the target in F) from the KCfg named cf.  One text for both; k_cl_diag's token
// stream is unchanged.
  Lin L;
  lin_load(lin + c * 35, L);
  double Km[NA], CL[NA * NA];
  mpc_kmpc<NP, NC>(cf, L, uk1[c], Km);
  closed_loop(L.a, Km, CL);
  if (poles) {
    double re[NA], im[NA];
    eig::eigvals(NA, CL, re, im);
    for (int i = 0; i < NA; ++i) {
      poles[(c * NA + i) * 2] = re[i];
      poles[(c * NA + i) * 2 + 1] = im[i];
    }
  }
  if (sv) {
    double s[NA];
    eig::singvals(NA, CL, s);
    for (int i = 0; i < NA; ++i) sv[c * NA + i] = s[i];
  }
