"""Shared by test_switches_oracle.py (CPU) and test_gpu_switches_edges.py / test_gpu_wide.py /
test_gpu_parity.py (GPU): the edit groups that push iterMPC's QP solve off its fast rank-2
sweep, and the causes a test can read back from the step's problem record.

Linearisation record [35]: a 0:6, Csoc 6:12, Dsoc 12, Cv 13:19, Dv 19, Cphi 20:26, Dphi 26,
bv 27, bphi 28, xhat 29:35 (include/mpcekf.h MPCEKF_LIN_*).
"""
import numpy as np

LIN_CSOC, LIN_DSOC = 6, 12          # MPCEKF_LIN_CSOC, MPCEKF_LIN_DSOC
NP5, NC2 = 5, 2
ALL_MASKS = [(c, v, e) for c in (0, 1) for v in (0, 1) for e in (0, 1)]
H_LO, H_HI = 2.0 ** -1020, 2.0 ** 1020   # hild_step's reciprocal domain (hild_rok)


def ncon(mask, Np=NP5, Nc=NC2):
    return (4 * Nc if mask[0] else 0) + (Np if mask[1] else 0) + (Np if mask[2] else 0) + Np


def rows_of(mask, Np=NP5, Nc=NC2):
    """All-on row numbers of the mask's compact stack (constraintsMPC.m's row order)."""
    r = list(range(4 * Nc)) if mask[0] else []
    if mask[1]:
        r += range(4 * Nc, 4 * Nc + Np)
    if mask[2]:
        r += range(4 * Nc + Np, 4 * Nc + 2 * Np)
    return np.array(r + list(range(4 * Nc + 2 * Np, 4 * Nc + 3 * Np)))


def groups(n):
    """Cell index % 8; of the plain cells, index % 16 == 8 is group 8 and index % 32 == 16
    group 9 (two plain cells stay in every wave)."""
    g = np.arange(n) % 8
    g[np.arange(n) % 16 == 8] = 8
    g[np.arange(n) % 32 == 16] = 9
    return g


def edit_records(lin, g):
    """The record edits of groups 1-6, 8 and 9, in place.  Group 6 alternates its two variants
    (6a: Dsoc = NaN, 6b: the SOC columns times 1e160) along the group's cells.
    Group 7 is a warm start (edit_lambda); group 0 stays plain."""
    lin[g == 1, 13:19] *= 1e300    # Cv: G_v rows overflow
    lin[g == 2, 19] = 1e200         # Dv: H_ii of the voltage rows overflows
    lin[g == 3, 20:26] = np.inf     # Cphi: G_e rows non-finite
    lin[g == 4, 27] = np.nan        # bv: a NaN bound
    lin[g == 5, 13:20] *= 1e-170    # G_v rows tiny
    six = np.nonzero(g == 6)[0]
    lin[six[0::2], LIN_DSOC] = np.nan
    lin[six[1::2], LIN_CSOC:LIN_DSOC + 1] *= 1e160
    lin[g == 8, 13:19] = np.inf     # Cv: G_v rows non-finite
    lin[g == 9, 13:20] *= 1e-156    # G_v rows tiny: H_ii subnormal, not 0
    return lin


def edit_lambda(lam, g):
    """Group 7: lambda = inf in the cell's last enabled row (a G_soc row under every mask);
    lam is the compact [n, ncon(mask)] warm start, edited in place."""
    lam[g == 7, -1] = np.inf
    return lam


def group_block(k):
    """The constraint block (index into the mask) a group's record edit lives in, or None
    for the groups every mask carries (SOC columns, warm start)."""
    return {1: 1, 2: 1, 5: 1, 3: 2, 4: 1, 8: 1, 9: 1}.get(k)


def structured_M(Hv, He, Hs, mask, Np=NP5, Nc=NC2):
    """constraintsMPC.m's M [nC, Nc] of the mask from the record's impulse responses."""
    def toep(h, sign):
        G = np.zeros((Np, Nc))
        for i in range(Np):
            for j in range(min(i + 1, Nc)):
                G[i, j] = h[i - j]
        return sign * G
    blocks = []
    if mask[0]:
        Cu = np.tril(np.ones((Nc, Nc)))
        blocks += [Cu, -Cu, np.eye(Nc), -np.eye(Nc)]
    if mask[1]:
        blocks.append(toep(Hv, 1.0))
    if mask[2]:
        blocks.append(toep(He, -1.0))
    blocks.append(toep(Hs, 1.0))
    return np.vstack(blocks)


def chol2_ok(E):
    """chol_n's verdict on a 2 x 2 E (the record's E, row-major [4]): both pivots > 0."""
    with np.errstate(all="ignore"):
        s0 = E[0]
        r01 = E[1] / np.sqrt(s0)
        s1 = E[3] - r01 * r01
        return bool(s0 > 0) and bool(s1 > 0)


def qp_cause(prob, mask, Np=NP5, Nc=NC2):
    """What the record of one cell (get_hild_problems()[0][:, c], Np = 5 layout: E 0:4, F 4:6,
    Hv 6:11, He 11:16, Hs 16:21) says about the sweep its QP takes: dict of
    E_finite, E_spd, M_finite (enabled rows), hii [nC] (M_i (E \\ M_i'), numpy; only
    meaningful for an SPD E with finite M) and hii_out (an enabled row's H_ii outside
    [2^-1020, 2^1020] and not 0)."""
    E = prob[0:4]
    Hv, He, Hs = prob[6:11], prob[11:16], prob[16:21]
    Mm = structured_M(Hv, He, Hs, mask, Np, Nc)
    out = dict(E_finite=bool(np.isfinite(E).all()), E_spd=chol2_ok(E), M_finite=bool(np.isfinite(Mm).all()))
    hii = np.full(Mm.shape[0], np.nan)
    out["X_finite"] = False
    if out["E_finite"] and out["E_spd"]:
        with np.errstate(all="ignore"):   # E \ M' by the 2 x 2 Cholesky factor, row by row
            r00 = np.sqrt(E[0])
            r01 = E[1] / r00
            r11 = np.sqrt(E[3] - r01 * r01)
            y0 = Mm[:, 0] / r00
            y1 = (Mm[:, 1] - r01 * y0) / r11
            x1 = y1 / r11
            x0 = (y0 - r01 * x1) / r00
            hii = Mm[:, 0] * x0 + Mm[:, 1] * x1
        out["X_finite"] = bool(np.isfinite(x0).all() and np.isfinite(x1).all())
    out["hii"] = hii
    a = np.abs(hii)
    out["hii_out"] = bool(((hii != 0) & ~((a >= H_LO) & (a <= H_HI))).any())
    return out


POISON = (np.inf, np.nan, 1e300, -0.0)


def poison_block(lin, fields):
    """A disabled block's record fields replaced by inf, NaN, 1e300 and -0.0 in four cell
    groups (cell index % 4), in place: "v" = Cv, Dv, bv; "eta" = Cphi, Dphi, bphi."""
    cols = list(range(13, 20)) + [27] if fields == "v" else list(range(20, 27)) + [28]
    k = np.arange(len(lin)) % 4
    for q, val in enumerate(POISON):
        lin[np.ix_(k == q, cols)] = val
    return lin
