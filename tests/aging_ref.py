"""The side-reaction rule of include/mpcekf.h (mpcekf_aging_begin) in numpy: every line one
separately rounded fp64 operation in the header's order, vectorised over cells, sequential over
steps.  dexp is rom.py's dexp (the kernels' and the C oracle's defined exp) over arrays, built
from np.floor, np.ldexp and plain operations only."""
import numpy as np

FIELDS = ("q_sum", "j_max", "j_max_step", "n_on", "steps", "nskip")
_P = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
      -1.65339022054652515390e-06, 4.13813679705723846039e-08)
_LN2_HI, _LN2_LO, _INVLN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00


def dexp(x0):
    x0 = np.asarray(x0, dtype=np.float64)
    nan, big, small = np.isnan(x0), x0 > 709.782712893384, x0 < -745.1332191019412
    x = np.where(nan | big | small, 0.0, x0)
    k = np.floor(x * _INVLN2 + 0.5)
    hi = x - k * _LN2_HI
    lo = k * _LN2_LO
    r = hi - lo
    t = r * r
    c = r - t * (_P[0] + t * (_P[1] + t * (_P[2] + t * (_P[3] + t * _P[4]))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    v = np.ldexp(y, k.astype(np.int32))
    return np.where(nan, x0, np.where(big, np.inf, np.where(small, 0.0, v)))


def new_record(nreact, n):
    """One source's record: per reaction q_sum, j_max, j_max_step, n_on; steps, nskip shared."""
    return dict(q_sum=np.zeros((nreact, n)), j_max=np.full((nreact, n), np.nan), j_max_step=np.zeros((nreact, n)),
                n_on=np.zeros((nreact, n)), steps=np.zeros(n), nskip=np.zeros(n))


def step(rec, phi, T, par, F, R, Tref):
    """One step of one source: phi, T [n]; par [nreact][5][n] (i0, U, alpha, Ea, gate).  Updates
    rec in place and returns the rate rows [nreact][n]."""
    phi, T = np.asarray(phi, dtype=np.float64), np.asarray(T, dtype=np.float64)
    nreact = par.shape[0]
    rate = np.empty((nreact, phi.shape[0]))
    TK = T + 273.15
    tt = (rec["steps"] + rec["nskip"]) + 1.0
    skip = np.isnan(phi)
    with np.errstate(all="ignore"):
        for r in range(nreact):
            i0, U, alpha, Ea, gate = par[r]
            eta = phi - U
            g = (alpha * F) / (R * TK)
            ar = dexp((Ea / R) * (1.0 / Tref - 1.0 / TK))
            j = (i0 * ar) * dexp(-(g * eta))
            take = (eta < gate) & np.isfinite(j)
            rec["q_sum"][r] = np.where(take, rec["q_sum"][r] + j, rec["q_sum"][r])
            rec["n_on"][r] = np.where(take, rec["n_on"][r] + 1.0, rec["n_on"][r])
            new = take & (np.isnan(rec["j_max"][r]) | (j > rec["j_max"][r]))
            rec["j_max"][r] = np.where(new, j, rec["j_max"][r])
            rec["j_max_step"][r] = np.where(new, tt, rec["j_max_step"][r])
            rate[r] = np.where(skip, np.nan, np.where(take, j, 0.0))
    rec["steps"] = np.where(skip, rec["steps"], rec["steps"] + 1.0)
    rec["nskip"] = np.where(skip, rec["nskip"] + 1.0, rec["nskip"])
    return rate


def run(phis, temps, par, F, R, Tref, rec=None):
    """phis, temps [nsteps][n] of one source -> (record, rate [nsteps][nreact][n])."""
    phis = np.asarray(phis, dtype=np.float64)
    rec = new_record(par.shape[0], phis.shape[1]) if rec is None else rec
    rate = np.empty((phis.shape[0], par.shape[0], phis.shape[1]))
    for t in range(phis.shape[0]):
        rate[t] = step(rec, phis[t], temps[t], par, F, R, Tref)
    return rec, rate


def params(n, reactions):
    """[{i0, U, alpha, Ea, gate (default inf)}] -> [nreact][5][n]"""
    par = np.empty((len(reactions), 5, n))
    for r, d in enumerate(reactions):
        for i, k in enumerate(("i0", "U", "alpha", "Ea", "gate")):
            par[r, i] = np.broadcast_to(np.asarray(d.get(k, np.inf) if k == "gate" else d[k], dtype=np.float64), (n,))
    return par
