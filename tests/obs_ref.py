"""Stateless numpy restatement of OB_step's obs output (OB_step.m:226-356).

TEST INFRASTRUCTURE ONLY.  ``oracle/oracle_np.ob_step`` returns Vcell alone; this file
restates the same simStep with every ``obs.`` assignment of the reference, from
oracle_np's own pieces (Cell, setup_inds, stable_two_nearest, mv, _sqrt) and in its
conventions: sequential sums from +0.0, no fused multiply-add, MATLAB max/min ignoring
NaN.  tests/test_obs_ref.py ties it to ob_step (Vcell bit for bit on a shared trajectory).

``ob_obs`` reads a state and changes nothing: the caller advances the state (ob_step, or
the library under test).
"""
from __future__ import annotations

import math

import numpy as np

from oracle_np import Cell, _sqrt, mv, setup_inds, stable_two_nearest

# every name assigned to ``obs.`` in OB_step.m:226-228 and 289-356, in the reference's order
OBS_FIELDS = ("negSOC", "posSOC", "cellSOC", "negIfdl", "posIfdl", "negIfdl0", "posIfdl3", "negIf", "posIf",
              "negIf0", "posIf3", "negIdl", "posIdl", "negThetass", "posThetass", "negThetass0", "posThetass3",
              "negPhise", "posPhise", "negPhise0", "Phie", "Thetae", "negPhis", "posPhis", "Vcell")


def _max(x, lo):
    """MATLAB max(x, lo) elementwise: a NaN entry gives lo."""
    x = np.asarray(x, dtype=float)
    return np.where(x >= lo, x, lo)


def _min(x, hi):
    x = np.asarray(x, dtype=float)
    return np.where(x <= hi, x, hi)


def ob_obs(rom, bigX_c, SOCnAvg, SOCpAvg, SOC0n, SOC0p, Iapp, Tc, handles=False, return_yk=False):
    """obs of one simStep (OB_step.m:188-357) on the pre-step state of one cell.

    bigX_c [NM, 6]: cellState.bigX, a row per model (column (tt-1)*ZZ+zz of the reference);
    SOCnAvg / SOCpAvg: cellState.SOCnAvg / SOCpAvg; SOC0n / SOC0p: cellState.SOC0n / SOC0p.
    Returns {field: float or 1-D array} with the fields of OBS_FIELDS; vector fields are in
    ROM row order (MATLAB's find), possibly empty.  return_yk: (obs, yk), yk the blended
    output vector of OB_step.m:285 (for the identities the tests check)."""
    cell = Cell(rom, handles)
    ind = setup_inds(rom)
    loc = np.asarray(rom.xloc, dtype=float)
    at = lambda nm, x: [i for i in ind[nm] if loc[i] == x][0]               # OB_step.m:131-137
    T = Tc + 273.15                                                         # OB_step.m:75
    F, R, Rc = cell.F, cell.R, cell.Rc
    theta0n, theta100n = cell.e["neg"].theta0, cell.e["neg"].theta100
    obs = {}
    obs["negSOC"] = float(SOCnAvg)                                          # OB_step.m:226
    obs["posSOC"] = float(SOCpAvg)                                          # OB_step.m:227
    obs["cellSOC"] = (SOCnAvg - theta0n) / (theta100n - theta0n)            # OB_step.m:228
    Zspts = np.sort(rom.SOC_pct / 100)                                      # OB_step.m:167
    Tspts = np.sort(rom.T_degC) + 273.15                                    # OB_step.m:166
    ZZ = rom.nZ
    if len(Zspts) > 1:                                                      # OB_step.m:251-259
        a, b = stable_two_nearest(np.abs(obs["cellSOC"] - Zspts))
        iZu, iZl = max(a, b), min(a, b)
    else:
        iZu = iZl = 0
    Zu, Zl = Zspts[iZu], Zspts[iZl]
    if len(Tspts) > 1:                                                      # OB_step.m:261-269
        a, b = stable_two_nearest(np.abs(T - Tspts))
        iTu, iTl = max(a, b), min(a, b)
    else:
        iTu = iTl = 0
    Tu, Tl = Tspts[iTu], Tspts[iTl]
    bigX_c = np.asarray(bigX_c, dtype=float)

    def yk_of(it, iz):
        C = np.array(rom.C[it, iz], dtype=float)
        C[ind["negPhise"], -1] = 0.0                                        # OB_step.m:178
        if ind["posPhise"]:
            C[ind["posPhise"], -1] = 0.0                                    # OB_step.m:179-181
        return mv(C, bigX_c[it * ZZ + iz]) + np.asarray(rom.D[it, iz], dtype=float) * Iapp   # OB_step.m:272-275

    yk1, yk2, yk3, yk4 = yk_of(iTl, iZl), yk_of(iTl, iZu), yk_of(iTu, iZl), yk_of(iTu, iZu)
    aZ = 0.0
    aT = 0.0
    if Zu != Zl:
        aZ = (obs["cellSOC"] - Zl) / (Zu - Zl)                              # OB_step.m:282
    if Tu != Tl:
        aT = (T - Tl) / (Tu - Tl)                                           # OB_step.m:283
    yk = (1 - aT) * ((1 - aZ) * yk1 + aZ * yk2) + aT * ((1 - aZ) * yk3 + aZ * yk4)   # OB_step.m:285
    obs["negIfdl"] = yk[ind["negIfdl"]]                                     # OB_step.m:289
    obs["posIfdl"] = yk[ind["posIfdl"]]                                     # OB_step.m:290
    obs["negIfdl0"] = yk[at("negIfdl", 0)]                                  # OB_step.m:291
    obs["posIfdl3"] = yk[at("posIfdl", 3)]                                  # OB_step.m:292
    obs["negIf"] = yk[ind["negIf"]]                                         # OB_step.m:294
    obs["posIf"] = yk[ind["posIf"]]                                         # OB_step.m:295
    obs["negIf0"] = yk[at("negIf", 0)]                                      # OB_step.m:296
    obs["posIf3"] = yk[at("posIf", 3)]                                      # OB_step.m:297
    obs["negIdl"] = yk[ind["negIdl"]]                                       # OB_step.m:299
    obs["posIdl"] = yk[ind["posIdl"]]                                       # OB_step.m:300
    clamp = lambda x: _min(_max(x, 1e-6), 1 - 1e-6)                         # OB_step.m:307-310
    obs["negThetass"] = clamp(yk[ind["negThetass"]] + SOC0n)                # OB_step.m:302,307
    obs["posThetass"] = clamp(yk[ind["posThetass"]] + SOC0p)                # OB_step.m:303,308
    obs["negThetass0"] = float(clamp(yk[at("negThetass", 0)] + SOC0n))      # OB_step.m:304,309
    obs["posThetass3"] = float(clamp(yk[at("posThetass", 3)] + SOC0p))      # OB_step.m:305,310
    UocpnAvg = cell.Uocp("neg", obs["negSOC"], T)                           # OB_step.m:313
    UocppAvg = cell.Uocp("pos", obs["posSOC"], T)                           # OB_step.m:314
    obs["negPhise"] = yk[ind["negPhise"]] + UocpnAvg                        # OB_step.m:315
    obs["posPhise"] = yk[ind["posPhise"]] + UocppAvg                        # OB_step.m:316
    obs["negPhise0"] = yk[at("negPhise", 0)] + UocpnAvg                     # OB_step.m:317
    Phie = np.zeros(len(ind["Phie"]) + 1)                                   # OB_step.m:320
    Phie[0] = -obs["negPhise0"]                                             # OB_step.m:321
    Phie[1:] = yk[ind["Phie"]] - obs["negPhise0"]                           # OB_step.m:322
    obs["Phie"] = Phie
    obs["Thetae"] = _max(yk[ind["Thetae"]] + 1, 1e-6)                       # OB_step.m:325-326
    k0n = cell.k0("neg", obs["negSOC"], T)                                  # OB_step.m:329
    k0p = cell.k0("pos", obs["posSOC"], T)                                  # OB_step.m:330
    i0n = k0n * _sqrt(obs["Thetae"][0] * (1 - obs["negThetass0"]) * obs["negThetass0"])    # OB_step.m:331
    i0p = k0p * _sqrt(obs["Thetae"][-1] * (1 - obs["posThetass3"]) * obs["posThetass3"])   # OB_step.m:332
    negEta0 = 2 * R * T / F * math.asinh(obs["negIf0"] / (2 * i0n))         # OB_step.m:333
    posEta3 = 2 * R * T / F * math.asinh(obs["posIf3"] / (2 * i0p))         # OB_step.m:334
    Uocpn0 = cell.Uocp("neg", obs["negThetass0"], T)                        # OB_step.m:337
    Uocpp3 = cell.Uocp("pos", obs["posThetass3"], T)                        # OB_step.m:338
    Rfn = cell.Rf("neg", obs["negSOC"], T)                                  # OB_step.m:339
    Rfp = cell.Rf("pos", obs["posSOC"], T)                                  # OB_step.m:340
    Vcell = (posEta3 - negEta0 + yk[ind["Phie"][-1]] + Uocpp3 - Uocpn0
             + (Rfp * obs["posIfdl3"] - Rfn * obs["negIfdl0"]))             # OB_step.m:341-342
    Vcell = Vcell - Rc * Iapp                                               # OB_step.m:344
    obs["negPhis"] = yk[ind["negPhis"]]                                     # OB_step.m:347
    obs["posPhis"] = yk[ind["posPhis"]] + Vcell                             # OB_step.m:348
    obs["Vcell"] = float(Vcell)                                             # OB_step.m:356
    for k in ("cellSOC", "negIfdl0", "posIfdl3", "negIf0", "posIf3", "negPhise0"):
        obs[k] = float(obs[k])
    assert tuple(obs) == OBS_FIELDS
    return (obs, yk) if return_yk else obs


def profile(rom, steps, Crate=2.0):
    """The fixed current profile of the obs tests and fixture, independent of any controller:
    a charge at -Q*Crate for the first half, a rest, then a short discharge pulse at +Q/2
    (currents of both signs and zero), per step, amperes."""
    u = np.zeros(steps)
    a, b = steps // 2, steps - max(steps // 6, 1)
    u[:a] = -rom.Q * Crate
    u[b:] = 0.5 * rom.Q
    return u
