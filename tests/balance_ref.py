"""The passive-balancing rule of include/mpcekf.h (mpcekf_balance_begin) restated in plain Python:
an explicit loop over steps, strings and cells, written from the header and nothing else.  Shared
by tests/test_balance_ref.py (hand-written cases) and tests/test_gpu_balance.py (the host-driven
loop); it never sees the code under test.

  step(ucmd, soc, S, i_bleed, dz_on, dz_off, compensate, state=None) -> dict

ucmd, soc: float64 [nsteps, ncells], each cell's own command and soc row of every step; S: cells
per string (ncells % S == 0; string g is the cells [g*S, (g+1)*S)); i_bleed, dz_on, dz_off:
float64 [ncells]; compensate: 0 / 1.  Returns u [nsteps, ncells], the applied current a_c (a
cell with a NaN command keeps its NaN); bleed [nsteps, ncells], b_c (NaN for a NaN command); zmin
[nsteps, ncells // S]; limiter [nsteps, ncells // S] int32 (-1: no non-NaN command); e
[nsteps, ncells], the effective commands; on [ncells] int, the flags after the last step; the
pack record nlim, steps, headroom and the balance record steps_on, q_bleed, switches, dz_max,
dz_last, bsteps (the header's STEPS), float64 [ncells] each.  state: the dict of an earlier call
to go on from (flags and records accumulate across calls).
"""
import numpy as np

PACK_FIELDS = ("nlim", "steps", "headroom")
FIELDS = ("steps_on", "q_bleed", "switches", "dz_max", "dz_last", "bsteps")
# FIELDS in the order of _lib.BALANCE_FIELDS: the record's last row is called "steps" there
LIB_NAMES = dict(zip(FIELDS, ("steps_on", "q_bleed", "switches", "dz_max", "dz_last", "steps")))


def reset(n):
    st = {k: np.zeros(n) for k in PACK_FIELDS + FIELDS}
    st["dz_max"] = np.full(n, np.nan)
    st["dz_last"] = np.full(n, np.nan)
    st["on"] = np.zeros(n, dtype=np.int64)
    return st


def step(ucmd, soc, S, i_bleed, dz_on, dz_off, compensate, state=None):
    ucmd = np.asarray(ucmd, dtype=np.float64)
    soc = np.asarray(soc, dtype=np.float64)
    nsteps, n = ucmd.shape
    S = int(S)
    if S < 1 or n % S:
        raise ValueError(f"balance_ref: series = {S} must be >= 1 and divide ncells = {n}")
    if compensate not in (0, 1):
        raise ValueError(f"balance_ref: compensate = {compensate!r}")
    i_bleed, dz_on, dz_off = (np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) for a in (i_bleed, dz_on, dz_off))
    nstr = n // S
    st = reset(n) if state is None else {k: np.array(state[k]) for k in PACK_FIELDS + FIELDS + ("on",)}
    on = st["on"]
    u = ucmd.copy()
    e = ucmd.copy()
    bleed = np.full((nsteps, n), np.nan)
    zmin = np.full((nsteps, nstr), np.nan)
    limiter = np.full((nsteps, nstr), -1, dtype=np.int32)
    nan = np.float64(np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(nsteps):
            for g in range(nstr):
                cells = range(g * S, (g + 1) * S)
                # 1. the smallest soc over the valid cells; a tie keeps the lower index
                valid = {c: (ucmd[t, c] == ucmd[t, c] and soc[t, c] == soc[t, c]) for c in cells}
                zm, have = nan, False
                for c in cells:
                    if valid[c] and (not have or soc[t, c] < zm):
                        zm, have = soc[t, c], True
                zmin[t, g] = zm
                # 2., 3. the flags, the bleed currents, the effective commands
                b = {}
                bleeding = {}
                for c in cells:
                    was = on[c]
                    if valid[c]:
                        d = soc[t, c] - zm                       # one rounded subtraction
                        if d >= dz_on[c]:
                            on[c] = 1
                        elif d <= dz_off[c]:
                            on[c] = 0
                        st["bsteps"][c] += 1.0
                        st["dz_last"][c] = d
                        if d == d and (st["dz_max"][c] != st["dz_max"][c] or d > st["dz_max"][c]):
                            st["dz_max"][c] = d
                    else:
                        on[c] = 0
                        st["dz_last"][c] = nan
                    if on[c] and not was:
                        st["switches"][c] += 1.0
                    bleeding[c] = bool(on[c]) and i_bleed[c] > 0
                    b[c] = i_bleed[c] if bleeding[c] else np.float64(0.0)
                    if bleeding[c]:
                        st["steps_on"][c] += 1.0
                        st["q_bleed"][c] = st["q_bleed"][c] + b[c]
                    x = ucmd[t, c]
                    e[t, c] = x - b[c] if (compensate and bleeding[c] and x < 0) else x
                    bleed[t, c] = b[c] if x == x else nan
                # 4. the limiter on e among the cells with a command; a tie keeps the lower index
                lim, m = -1, nan
                for i, c in enumerate(cells):
                    if ucmd[t, c] != ucmd[t, c]:
                        continue
                    if lim < 0 or e[t, c] > m:
                        lim, m = i, e[t, c]
                limiter[t, g] = lim
                if lim < 0:
                    continue                                     # the string writes nothing
                # 5., 6. the applied currents and the pack record
                for i, c in enumerate(cells):
                    if ucmd[t, c] != ucmd[t, c]:
                        continue
                    u[t, c] = m + b[c] if bleeding[c] else m     # one rounded addition
                    st["steps"][c] += 1.0
                    if i == lim:
                        st["nlim"][c] += 1.0
                    h = m - e[t, c]                              # one rounded subtraction
                    if np.isfinite(h):
                        st["headroom"][c] = st["headroom"][c] + h
    return dict(u=u, bleed=bleed, zmin=zmin, limiter=limiter, e=e, **st)
