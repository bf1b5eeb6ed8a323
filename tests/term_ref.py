"""The termination rule of include/mpcekf.h (mpcekf_term_begin) in plain numpy, written from the
header only: one call of step() is the rule of one fused step for every cell.

State per cell: OPEN (0), LATCHED (1) or DEAD (2); the record's fields (FIELDS, the header's
MPCEKF_TM_* in order) and the taper counter (armed, run).  The string flag of rule b is what the
cells' states were when the step began, i.e. after step t - 1: a cell that latches in step t does
not take its string-mates with it before step t + 1."""
import numpy as np

FIELDS = ("state", "done_step", "reason", "soc_done", "u_done", "T_done", "rest", "steps")
OPEN, LATCHED, DEAD = 0, 1, 2
R_SOC, R_TAPER, R_TEMP, R_STRING = 1, 2, 4, 8


def reset(n):
    """The state mpcekf_term_begin leaves: every cell OPEN, the record empty, t = 0."""
    st = {k: np.zeros(n) for k in FIELDS}
    for k in ("soc_done", "u_done", "T_done"):
        st[k] = np.full(n, np.nan)
    st["armed"] = np.zeros(n, dtype=bool)
    st["run"] = np.zeros(n, dtype=np.int64)
    st["t"] = 0
    return st


def _per_cell(v, n):
    return np.broadcast_to(np.asarray(np.nan if v is None else v, dtype=np.float64), (n,))


def step(st, z, u, T, soc_stop=None, i_taper=None, hold=1, T_cut=None, series=None):
    """One fused step's rule.  z, u, T [n]: the step's soc row, the cells' own commands and the
    temperature the step used.  Returns (the commands after the rule: +0.0 for a latched cell
    whose command is not NaN, the next state).  st is not modified."""
    z, u, T = (np.asarray(a, dtype=np.float64) for a in (z, u, T))
    n = z.shape[0]
    soc_stop, i_taper, T_cut = (_per_cell(v, n) for v in (soc_stop, i_taper, T_cut))
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    t = st["t"] = st["t"] + 1
    was_open = st["state"] == OPEN
    st["steps"][was_open] += 1
    # a. a NaN input kills the cell
    dead = was_open & (np.isnan(z) | np.isnan(u))
    st["state"][dead] = DEAD
    st["done_step"][dead] = t
    # b. the string flag: the strings that held a latched cell when the step began
    follow = np.zeros(n, dtype=bool)
    if series is not None and series > 1:
        flag = (st["state"].reshape(-1, series) == LATCHED).any(axis=1)   # DEAD set above is not LATCHED
        follow = was_open & ~dead & np.repeat(flag, series)
    # c. the criteria
    c = was_open & ~dead & ~follow
    with np.errstate(invalid="ignore"):
        au = np.fabs(u)
        big = c & (au > i_taper)
        small = c & ~big & st["armed"] & (au <= i_taper)
        st["armed"][big] = True
        st["run"][big] = 0
        st["run"][small] += 1
        st["run"][c & ~big & ~small] = 0
        reason = (np.where(z >= soc_stop, R_SOC, 0) | np.where(st["run"] >= hold, R_TAPER, 0)
                  | np.where(T >= T_cut, R_TEMP, 0))
    reason = np.where(c, reason, 0)
    reason[follow] = R_STRING
    latch = reason != 0
    st["state"][latch] = LATCHED
    st["done_step"][latch] = t
    st["reason"][latch] = reason[latch]
    st["soc_done"][latch] = z[latch]
    st["u_done"][latch] = u[latch]
    st["T_done"][latch] = T[latch]
    # a latched cell rests, one latched in this step included; a NaN command is left alone
    rest = (st["state"] == LATCHED) & ~np.isnan(u)
    out = u.copy()
    out[rest] = 0.0
    st["rest"][rest] += 1
    return out, st


def n_open(st):
    return int((st["state"] == OPEN).sum())


def record(st):
    return {k: st[k] for k in FIELDS}
