"""The series-string rule of include/mpcekf.h (mpcekf_pack_begin) restated in plain Python: an
explicit loop over steps, strings and cells, written from the header and nothing else.  Shared
by tests/test_pack_ref.py (hand-written cases) and tests/test_gpu_pack.py (the host-driven
loop); it never sees the code under test.

  reduce(ucmd, S, state=None) -> dict(u, limiter, nlim, steps, headroom)

ucmd: float64 [nsteps, ncells], each cell's own command of every step; S: cells per string
(ncells % S == 0; string g is the cells [g*S, (g+1)*S)).  u [nsteps, ncells]: the applied
current (the limiter's command, bit for bit, for every cell of the string whose own command is
not NaN; an excluded cell keeps its NaN); limiter [nsteps, ncells // S] int32: the in-string
index, or -1 for a string with no non-NaN command; nlim, steps, headroom float64 [ncells]: the
record.  state: the record of an earlier reduce to go on from (accumulation across calls).
"""
import numpy as np

FIELDS = ("nlim", "steps", "headroom")


def reset(n):
    return {k: np.zeros(n) for k in FIELDS}


def reduce(ucmd, S, state=None):
    ucmd = np.asarray(ucmd, dtype=np.float64)
    nsteps, n = ucmd.shape
    S = int(S)
    if S < 1 or n % S:
        raise ValueError(f"pack_ref: series = {S} must be >= 1 and divide ncells = {n}")
    nstr = n // S
    u = ucmd.copy()
    limiter = np.full((nsteps, nstr), -1, dtype=np.int32)
    rec = reset(n) if state is None else {k: np.array(state[k], dtype=np.float64) for k in FIELDS}
    for t in range(nsteps):
        for g in range(nstr):
            lim, m = -1, np.float64(np.nan)
            for i in range(S):
                x = ucmd[t, g * S + i]
                if x != x:
                    continue            # NaN: excluded
                if lim < 0 or x > m:    # by value (-0.0 == +0.0); a tie keeps the lower index
                    lim, m = i, x
            limiter[t, g] = lim
            if lim < 0:
                continue                # the string writes nothing
            for i in range(S):
                c = g * S + i
                x = ucmd[t, c]
                if x != x:
                    continue
                u[t, c] = m
                rec["steps"][c] += 1.0
                if i == lim:
                    rec["nlim"][c] += 1.0
                with np.errstate(invalid="ignore"):
                    d = m - x           # one rounded subtraction
                if np.isfinite(d):
                    rec["headroom"][c] = rec["headroom"][c] + d   # one rounded addition, in step order
    return dict(u=u, limiter=limiter, **rec)
