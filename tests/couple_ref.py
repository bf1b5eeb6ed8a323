"""Numpy restatement of include/mpcekf.h's heat conduction between neighbouring cells of a pack
string (mpcekf_thermal_couple): one numpy operation per rounded fp64 operation, in the header's
order.  model_step / restate extend the functions of the same names in tests/test_gpu_thermal.py
(copied here; that file restates the uncoupled model) by the links.  Host numpy only: nothing
here comes from the library.
"""
import numpy as np

COUPLE_FIELDS = ("NB_SUM", "DT_MAX", "DT_MAX_STEP")
THERMAL_FIELDS = ("T", "T_max", "T_max_step", "T_min", "heat_sum", "steps", "nheld")


def conduct(T, r_link, S):
    """One step's neighbour terms from the temperatures T [n] the step used.
    Returns (qn, nl, dl, dr, has_l, has_r): dl / dr are NaN where the side has no finite link."""
    n = T.shape[0]
    c = np.arange(n)
    p = c % S
    r_link = np.asarray(r_link, dtype=np.float64)
    rl = np.where(p > 0, np.roll(r_link, 1), np.inf)          # r_link[c-1]
    rr = np.where(p < S - 1, r_link, np.inf)                  # r_link[c]
    has_l, has_r = np.isfinite(rl), np.isfinite(rr)
    Tl, Tr = np.roll(T, 1), np.roll(T, -1)
    with np.errstate(all="ignore"):
        qn = np.zeros(n)                                      # +0.0
        dl = Tl - T
        qn = np.where(has_l, qn + dl / np.where(has_l, rl, 1.0), qn)
        dr = Tr - T
        qn = np.where(has_r, qn + dr / np.where(has_r, rr, 1.0), qn)
    nl = has_l.astype(np.int64) + has_r.astype(np.int64)
    return qn, nl, np.where(has_l, dl, np.nan), np.where(has_r, dr, np.nan), has_l, has_r


def model_step(T, i, v, socn, p, ocv, th0n, th100n, Ts, qn=None, nl=None):
    """The thermal recurrence with the neighbours' heat flow.  Returns (z, q, Tn, advanced)."""
    nocv = ocv.shape[0]
    with np.errstate(all="ignore"):
        z = (socn - th0n) / (th100n - th0n)
        zc = np.where(z > 0.0, z, 0.0)
        zc = np.where(zc < 1.0, zc, 1.0)
        s = zc * float(nocv - 1)
        j = np.minimum(s.astype(np.int64), nocv - 2)
        f = s - j.astype(np.float64)
        U = ocv[j] + f * (ocv[j + 1] - ocv[j])
        q = i * (U - v)
        loss = (T - p["Tamb"]) / p["Rth"]
        Tn = T + ((q - loss) * Ts) / p["Cth"]                 # the uncoupled line
        if qn is not None:
            Tc = T + (((q - loss) + qn) * Ts) / p["Cth"]
            Tn = np.where(nl == 0, Tn, Tc)
        ok = np.isfinite(Tn) & (Tn <= 100.0)
    return z, q, Tn, ok


def new_records(n):
    th = dict(T_max=np.full(n, np.nan), T_max_step=np.zeros(n), T_min=np.full(n, np.nan),
              heat_sum=np.zeros(n), steps=np.zeros(n), nheld=np.zeros(n))
    cp = dict(NB_SUM=np.zeros(n), DT_MAX=np.full(n, np.nan), DT_MAX_STEP=np.zeros(n))
    return th, cp


def fold(cp, step, qn, nl, dl, dr, has_l, has_r):
    """The coupling's record after one step with index `step` [n]."""
    add = (nl > 0) & np.isfinite(qn)
    with np.errstate(all="ignore"):
        cp["NB_SUM"] = np.where(add, cp["NB_SUM"] + np.where(add, qn, 0.0), cp["NB_SUM"])
        for has, d in ((has_l, dl), (has_r, dr)):             # the left link first
            a = np.abs(d)
            up = has & (np.isnan(cp["DT_MAX"]) | (a > cp["DT_MAX"]))
            cp["DT_MAX"] = np.where(up, a, cp["DT_MAX"])
            cp["DT_MAX_STEP"] = np.where(up, step, cp["DT_MAX_STEP"])


def restate(Ts, th0n, th100n, p, ocv, r_link, S, T0, uk0, u, v, negsoc, socn_end, rec=None, error=None):
    """The coupled model over a call's trajectories: u, v, negsoc [nsteps, n] as the library
    returned them (i of step t is u[t-1], uk0 for the first; SOCnAvg after step t is negsoc[t+1],
    socn_end for the last).  rec: (thermal record, coupling record) to continue, None: fresh.
    error [n] bool: cells whose v counts as NaN (MPCEKF_ST_ERROR), None: v as given.
    Returns temp, heat, cond [nsteps, n], the thermal record (with T) and the coupling record."""
    nsteps, n = u.shape
    T = np.array(T0, dtype=np.float64)
    th, cp = rec if rec is not None else new_records(n)
    temp, heat, cond = np.empty((nsteps, n)), np.empty((nsteps, n)), np.empty((nsteps, n))
    for t in range(nsteps):
        i = uk0 if t == 0 else u[t - 1]
        socn = negsoc[t + 1] if t + 1 < nsteps else socn_end
        vt = v[t] if error is None else np.where(error, np.nan, v[t])
        qn, nl, dl, dr, has_l, has_r = conduct(T, r_link, S)
        z, q, Tn, ok = model_step(T, i, vt, socn, p, ocv, th0n, th100n, Ts, qn, nl)
        step = (th["steps"] + th["nheld"]) + 1.0
        up = np.isnan(th["T_max"]) | (T > th["T_max"])
        th["T_max"], th["T_max_step"] = np.where(up, T, th["T_max"]), np.where(up, step, th["T_max_step"])
        th["T_min"] = np.where(np.isnan(th["T_min"]) | (T < th["T_min"]), T, th["T_min"])
        th["heat_sum"] = np.where(np.isfinite(q), th["heat_sum"] + np.where(np.isfinite(q), q, 0.0), th["heat_sum"])
        th["steps"], th["nheld"] = th["steps"] + ok, th["nheld"] + ~ok
        fold(cp, step, qn, nl, dl, dr, has_l, has_r)
        temp[t], heat[t], cond[t] = T, q, qn
        T = np.where(ok, Tn, T)
    th["T"] = T
    return temp, heat, cond, th, cp
