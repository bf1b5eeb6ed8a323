"""The charger rule of include/mpcekf.h (mpcekf_charger_begin) restated in plain Python: an
explicit loop over steps, strings and cells, written from the header and nothing else.  Steps 1 to
4 of the balance rule and the pack's limiter come from tests/balance_ref.py / tests/pack_ref.py,
which restate those sections.  Shared by tests/test_charger_ref.py (hand-written cases) and
tests/test_gpu_charger.py (the host-driven loop); it never sees the code under test.

  tree_sum(x) -> float64          the header's fixed tree over x[0 .. S-1]
  string_voltage(u, v) -> (V, nvalid)
  caps(m, V, i_max, p_max) -> (m', capby)
  step(ucmd, soc, v, S, i_max, p_max, balance=None, state=None) -> dict

ucmd, soc, v: float64 [nsteps, ncells], each cell's own command, soc row and plant voltage (s.vk)
of every step; S: cells per string; i_max, p_max: a scalar or float64 [ncells // S] (NaN: off);
balance: None or (i_bleed, dz_on, dz_off, compensate).  Returns u [nsteps, ncells], the applied
current; limiter [nsteps, nstrings] int32 (-1: no command, -2: a cap set the current); vstr, istr
[nsteps, nstrings]; capby [nsteps, nstrings] int32; mraw [nsteps, nstrings], the string current
before the caps (NaN: none); with a balancer bleed, zmin; and "st", the state to go on from:
st["pack"] (nlim, steps, headroom), st["charger"] (FIELDS) and st["bal"] (balance_ref's state, or
None).
"""
import numpy as np

import balance_ref as br
import pack_ref as pr

FIELDS = ("steps", "ncap_i", "ncap_p", "q", "e", "curtail", "p_min", "v_peak", "nvalid_min")


def tree_sum(x):
    """Level j = 0, 1, .. while 2^j < S: x[i] += x[i + 2^j] for every i that is a multiple of
    2^(j+1) with i + 2^j < S; the result is x[0]."""
    x = [np.float64(a) for a in x]
    S = len(x)
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while (1 << j) < S:
            for i in range(0, S, 2 << j):
                if i + (1 << j) < S:
                    x[i] = x[i] + x[i + (1 << j)]        # one rounded addition
            j += 1
    return x[0]


def string_voltage(u, v):
    """Steps 1 and 2 for one string: (V_g, nvalid_g)."""
    zero = np.float64(0.0)
    terms, nvalid = [], 0
    for uc, vc in zip(u, v):
        if uc == uc and vc == vc:
            terms.append(np.float64(vc) + zero)          # -0.0 becomes +0.0
            nvalid += 1
        else:
            terms.append(zero)
    return tree_sum(terms), nvalid


def caps(m, V, i_max, p_max):
    """Step 4 for a string with a current m: (m', capby)."""
    cap, by = None, 0
    if i_max == i_max:
        cap, by = -np.float64(i_max), 1
    if p_max == p_max and V > 0:
        with np.errstate(over="ignore"):
            cp = -(np.float64(p_max) / np.float64(V))    # one rounded division, an exact negation
        if cap is None or cp > cap:                      # a tie keeps the current cap
            cap, by = cp, 2
    if cap is not None and cap > m:
        return cap, by
    return m, 0


def reset(n, S, balance=False):
    nstr = n // S
    ch = {k: np.zeros(nstr) for k in FIELDS}
    for k in ("p_min", "v_peak", "nvalid_min"):
        ch[k] = np.full(nstr, np.nan)
    return dict(pack=pr.reset(n), charger=ch, bal=br.reset(n) if balance else None)


def step(ucmd, soc, v, S, i_max, p_max, balance=None, state=None):
    ucmd = np.asarray(ucmd, dtype=np.float64)
    soc = np.asarray(soc, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    nsteps, n = ucmd.shape
    S = int(S)
    if S < 1 or n % S:
        raise ValueError(f"charger_ref: series = {S} must be >= 1 and divide ncells = {n}")
    nstr = n // S
    i_max, p_max = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nstr,)) for a in (i_max, p_max))
    st = reset(n, S, balance is not None) if state is None else state
    pk = {k: np.array(st["pack"][k], dtype=np.float64) for k in pr.FIELDS}
    ch = {k: np.array(st["charger"][k], dtype=np.float64) for k in FIELDS}
    out = {}
    if balance is not None:       # steps 1 to 4 of the balance rule: e, b, the limiter on e
        r = br.step(ucmd, soc, S, *balance, state=st["bal"])
        bal = {k: r[k] for k in br.PACK_FIELDS + br.FIELDS + ("on",)}
        e, lim0, b = r["e"], r["limiter"], r["bleed"]
        out["bleed"], out["zmin"] = r["bleed"], r["zmin"]
    else:                         # the pack's rule: e = u, no bleeder
        r = pr.reduce(ucmd, S)
        bal = None
        e, lim0, b = ucmd, r["limiter"], np.zeros_like(ucmd)
    u = ucmd.copy()
    limiter = lim0.copy()
    vstr = np.zeros((nsteps, nstr))
    istr = np.full((nsteps, nstr), np.nan)
    mraw = np.full((nsteps, nstr), np.nan)
    capby = np.full((nsteps, nstr), -1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(nsteps):
            for g in range(nstr):
                cells = range(g * S, (g + 1) * S)
                V, nvalid = string_voltage(ucmd[t, g * S:(g + 1) * S], v[t, g * S:(g + 1) * S])
                vstr[t, g] = V
                lim = int(lim0[t, g])
                if lim < 0:
                    continue                              # no string current: nothing written, nothing counted
                m = e[t, g * S + lim]
                m2, by = caps(m, V, i_max[g], p_max[g])
                mraw[t, g], istr[t, g], capby[t, g] = m, m2, by
                if by:
                    limiter[t, g] = -2
                for i, c in enumerate(cells):
                    if ucmd[t, c] != ucmd[t, c]:
                        continue
                    u[t, c] = m2 + b[t, c] if b[t, c] > 0 else m2   # one rounded addition for a bleeding cell
                    pk["steps"][c] += 1.0
                    if i == lim and not by:
                        pk["nlim"][c] += 1.0
                    h = m2 - e[t, c]
                    if np.isfinite(h):
                        pk["headroom"][c] = pk["headroom"][c] + h
                ch["steps"][g] += 1.0
                if by == 1:
                    ch["ncap_i"][g] += 1.0
                if by == 2:
                    ch["ncap_p"][g] += 1.0
                if np.isfinite(m2):
                    ch["q"][g] = ch["q"][g] + m2
                p = V * m2                                # one rounded product
                if np.isfinite(p):
                    ch["e"][g] = ch["e"][g] + p
                d = m2 - m
                if np.isfinite(d):
                    ch["curtail"][g] = ch["curtail"][g] + d
                if p == p and (ch["p_min"][g] != ch["p_min"][g] or p < ch["p_min"][g]):
                    ch["p_min"][g] = p
                if V == V and (ch["v_peak"][g] != ch["v_peak"][g] or V > ch["v_peak"][g]):
                    ch["v_peak"][g] = V
                if ch["nvalid_min"][g] != ch["nvalid_min"][g] or nvalid < ch["nvalid_min"][g]:
                    ch["nvalid_min"][g] = float(nvalid)
    out.update(u=u, limiter=limiter, vstr=vstr, istr=istr, capby=capby, mraw=mraw,
               st=dict(pack=pk, charger=ch, bal=bal))
    return out
