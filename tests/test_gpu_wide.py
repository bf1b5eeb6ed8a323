"""GPU parity at the wide horizons Np = 20 / Nc = 10 (BASELINE.json configs[4]).

The wide MPC stage (mpcekf_wide.hip: k_mpc_wide, k_hild_wide 8-lane groups,
k_hild_wide_slow, k_mpc_wide_finish) evaluates oracle/mpcekf_oracle.c's defined
order, including the lane-tree row sums of hild_row_t and orc_hildreth's one-row
lookahead, and the plant/EKF
upstream of it share the oracle's defined arithmetic (asinh included), so every
comparison with the C oracle is bitwise.
"""
import numpy as np
import pytest

from conftest import batch_inputs

pytestmark = pytest.mark.gpu

NP, NC = 20, 10
NCON = 4 * NC + 3 * NP
RTOL_TIGHT = 1e-9
RTOL_NORTH_STAR = 1e-6


def _rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    d[both_nan] = 0.0
    d[np.isnan(d)] = np.inf
    return d


@pytest.fixture(scope="module")
def M(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


def _cfg(M, **kw):
    return M.make_config(Np=NP, Nc=NC, **kw)


def test_wide_closed_loop_matches_oracle(rom, oc, M):
    """64 batch cells x 300 steps (SURVEY.md §8(d) inputs)."""
    n, steps = 64, 300
    soc0, tc = batch_inputs(n, seed=41)
    ref = oc.run(rom, soc0, tc, steps, nthreads=8, Np=NP, Nc=NC)
    out = M.runMPC(rom, soc0, tc, steps, cfg=_cfg(M))
    np.testing.assert_array_equal(out["status"], ref["status"])
    for k in ("u", "v", "soc", "phise", "nexec"):
        assert np.array_equal(out[k], ref[k], equal_nan=k != "nexec"), k


NEAR_SOC0 = np.array([88.0, 90.0, 93.0, 94.0, 94.5, 95.0, 96.0, 10.0, 50.0, 70.0, 80.0, 94.9, 95.1, 92.0, 25.0, 60.0])
NEAR_TC = np.array([25.0, 22.0, 25.0, 20.0, 30.0, 25.0, 25.0, 25.0, 28.0, 21.0, 35.0, 15.0, 25.0, 33.0, 20.0, 26.0])


def test_wide_closed_loop_near_limit(rom, oc, M):
    """Cells started at 88-96 % SOC: hildreth.m runs into maxIter on most steps and the
    zero G_soc row meets gamma <= 0 (the exact inf/NaN path, k_hild_wide_slow).  Closed
    loop, 400 steps, bitwise against the oracle (round 1 could only check this open loop:
    the plant's libm asinh made the chaotic maxIter regime diverge)."""
    steps = 400
    ref = oc.run(rom, NEAR_SOC0, NEAR_TC, steps, nthreads=8, Np=NP, Nc=NC)
    out = M.runMPC(rom, NEAR_SOC0, NEAR_TC, steps, cfg=_cfg(M))
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert (out["nexec"] == 100).sum() > steps  # the maxIter regime is really exercised
    for k in ("u", "v", "soc", "phise", "nexec"):
        assert np.array_equal(out[k], ref[k], equal_nan=k != "nexec"), k


def test_wide_mpc_stage_open_loop_near_limit(rom, oc, M):
    """The MPC stage entry point on the near-limit cells, open loop:
    every step the GPU's own linearisation record, mpcData.uk_1 and warm start go
    through iterMPC on the GPU and in the oracle, which must agree bit for bit (uk,
    nexec, lambda).  Near the 95 % limit the zero G_soc row meets gamma <= 0, the
    exact inf/NaN path (k_hild_wide_slow)."""
    soc0, tc = NEAR_SOC0, NEAR_TC
    n, steps = len(soc0), 120
    with M.Context(rom, n, _cfg(M)) as ctx:
        ctx.init_cells(soc0, tc)
        uk = np.zeros(n)
        saw_maxiter = False
        for k in range(steps):
            v = ctx.OB_step(uk)
            zk, _, xind = ctx.iterEKF(v, uk)
            lin = ctx.EKFmatsHandler(zk, xind)
            st = ctx.get_state()
            uk_r, ne_r, u1_r, lam_r = oc.mpc_lin(rom, lin, zk[:, -1], st["scal"][:, 5], st["lam"], Np=NP, Nc=NC)
            uk, ne = ctx.iterMPC(lin, zk[:, -1])
            np.testing.assert_array_equal(ne, ne_r, err_msg=f"step {k}")
            np.testing.assert_array_equal(uk, uk_r, err_msg=f"step {k}")
            np.testing.assert_array_equal(ctx.get_state()["lam"], lam_r, err_msg=f"step {k}")
            saw_maxiter = saw_maxiter or (ne == 100).any()
        assert saw_maxiter


def test_wide_mpc_stage_edge_records(rom, oc, M):
    """iterMPC on linearisation records built to leave k_hild_wide's fast form, next to
    plain ones: overflowing G_v rows and an infinite Cphi (non-finite M: k_hild_prep hands
    the cell to k_hild_wide_slow, which forms X and H_ii from R first), H_ii beyond 2^400
    and below 2^-400 (k_hild_wide's domain check after it formed X in its prologue), a NaN
    bound.  uk, nexec and lambda bitwise against the oracle (NaN where the oracle has NaN)."""
    n = 64
    soc0, tc = batch_inputs(n, seed=49)
    with M.Context(rom, n, _cfg(M)) as ctx:
        ctx.init_cells(soc0, tc)
        uk = np.zeros(n)
        for _ in range(4):
            v = ctx.OB_step(uk)
            zk, _, xind = ctx.iterEKF(v, uk)
            lin = ctx.EKFmatsHandler(zk, xind)
            uk, _ = ctx.iterMPC(lin, zk[:, -1])
        v = ctx.OB_step(uk)
        zk, _, xind = ctx.iterEKF(v, uk)
        lin = np.array(ctx.EKFmatsHandler(zk, xind), dtype=np.float64)
        g = np.arange(n) % 8
        lin[g == 1, 13:19] *= 1e300   # Cv: G_v rows overflow
        lin[g == 2, 19] = 1e200        # Dv: H_ii overflows
        lin[g == 3, 20:26] = np.inf    # Cphi: G_e rows non-finite
        lin[g == 4, 27] = np.nan       # bv: a NaN bound
        lin[g == 5, 13:20] *= 1e-170   # G_v rows tiny: H_ii below 2^-400
        zend = zk[:, -1]
        st = ctx.get_state()
        uk_r, ne_r, _, lam_r = oc.mpc_lin(rom, lin, zend, st["scal"][:, 5], st["lam"], Np=NP, Nc=NC)
        uk, ne = ctx.iterMPC(lin, zend)
        lam = ctx.get_state()["lam"]
    for k, (a, b) in {"uk": (uk, uk_r), "lam": (lam, lam_r)}.items():
        assert np.array_equal(a, b, equal_nan=True), (k, np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0][:8])
    np.testing.assert_array_equal(ne, ne_r)


DU_MAX_NEG = -1e7   # Ru = |F| / (2 du_max sqrt(Nc)) - sigma_min < -sigma_min: E finite, indefinite


def test_wide_mpc_stage_rejected_E(rom, oc, M):
    """iterMPC at Np = 20 / Nc = 10 on an E that Cholesky rejects, next to plain cells; uk,
    nexec and lambda bitwise against oc.mpc_lin(..., Np=20, Nc=10).

    Group 6 (cell % 8 == 6), alternating Dsoc = NaN and the SOC columns times 1e160: Hs, F,
    G'G, Ru and E are NaN, so DU = -E\\F (mpcekf_wide.hip:243) is NaN, no row test `acc - g > 0`
    (:259, :282, :306, :319) holds and k_mpc_wide returns at :324-335 with hflag = 0 (:168):
    both variants are no-QP cells with uk NaN and never reach k_hild_prep -- the oracle alone
    says the same (nexec = 0; tests/test_switches_oracle.py).  No edit of the SOC columns gives
    a non-SPD E with a non-NaN DU, so the input that does reach hflag = 3 is a negative du_max:
    the input weight Ru falls below -sigma_min(G'G), E = 2 (G'G + Ru I) is finite and indefinite
    on every cell, k_mpc_wide sets hflag = 1 (:337), k_hild_prep's chol_n rejects E and sets
    hflag = 3 (:418-419), and k_hild_wide_slow rebuilds K, X and H_ii by lu_solve_n (:975-1000).
    Group 7: lambda0 = inf in the last G_soc row, zk(end) at 0.9497 so that the SOC rows bind
    (hflag 1 -> the exact path)."""
    n = 64
    soc0, tc = batch_inputs(n, seed=49)
    with M.Context(rom, n, _cfg(M)) as ctx:
        ctx.init_cells(soc0, tc)
        uk = np.zeros(n)
        for _ in range(4):
            v = ctx.OB_step(uk)
            zk, _, xind = ctx.iterEKF(v, uk)
            lin = ctx.EKFmatsHandler(zk, xind)
            uk, _ = ctx.iterMPC(lin, zk[:, -1])
        v = ctx.OB_step(uk)
        zk, _, xind = ctx.iterEKF(v, uk)
        clean = np.array(ctx.EKFmatsHandler(zk, xind), dtype=np.float64)
        st = ctx.get_state()
        g = np.arange(n) % 8
        lin = clean.copy()
        six = np.nonzero(g == 6)[0]
        lin[six[0::2], 12] = np.nan     # Dsoc
        lin[six[1::2], 6:13] *= 1e160   # Csoc, Dsoc
        zend = zk[:, -1].copy()
        zend[g == 7] = 0.9497
        lam0 = st["lam"].copy()
        lam0[g == 7, -1] = np.inf
        ctx.set_state(dict(st, lam=lam0))
        uk_r, ne_r, _, lam_r = oc.mpc_lin(rom, lin, zend, st["scal"][:, 5], lam0, Np=NP, Nc=NC)
        uk, ne = ctx.iterMPC(lin, zend)
        lam = ctx.get_state()["lam"]
    assert (ne_r[six] == 0).all() and np.isnan(uk_r[six]).all() and (ne_r[g == 7] > 0).all()
    print(f"\nWIDE g6 nexec {ne[six].tolist()} g7 nexec {ne[g == 7].tolist()}")
    for k, (a, b) in {"uk": (uk, uk_r), "lam": (lam, lam_r)}.items():
        assert np.array_equal(a, b, equal_nan=True), (k, np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0][:8])
    np.testing.assert_array_equal(ne, ne_r)
    # the finite indefinite E: the clean record and state through a du_max < 0 context
    import oracle_np
    for c in range(0, n, 8):
        _, G = oracle_np.pred_mat(clean[c, 0:6], clean[c, 6:12], clean[c, 12], NP, NC)
        e = 95.0 - oracle_np.pred_mat(clean[c, 0:6], clean[c, 6:12], clean[c, 12], NP, NC)[0] @ np.append(clean[c, 29:35], st["scal"][c, 5])
        GtG = G.T @ G
        Ru = np.linalg.norm(-2 * G.T @ e) / (2 * DU_MAX_NEG * np.sqrt(NC)) - np.linalg.eigvalsh(GtG)[0]
        assert np.linalg.eigvalsh(2 * (GtG + Ru * np.eye(NC)))[0] < 0, c
    with M.Context(rom, n, _cfg(M, du_max=DU_MAX_NEG)) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_state(st)
        uk_r, ne_r, _, lam_r = oc.mpc_lin(rom, clean, zk[:, -1], st["scal"][:, 5], st["lam"], Np=NP, Nc=NC,
                                          du_max=DU_MAX_NEG)
        uk, ne = ctx.iterMPC(clean, zk[:, -1])
        lam = ctx.get_state()["lam"]
    assert (ne_r > 0).all()   # every cell set up a QP (hflag 1 -> 3)
    print(f"WIDE du_max<0 nexec {int(ne.min())}..{int(ne.max())}")
    for k, (a, b) in {"uk": (uk, uk_r), "lam": (lam, lam_r)}.items():
        assert np.array_equal(a, b, equal_nan=True), (k, np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0][:8])
    np.testing.assert_array_equal(ne, ne_r)


def test_wide_stage_entry_points_match_fused(rom, M):
    n, steps = 128, 12
    soc0, tc = batch_inputs(n, seed=43)
    cfg = _cfg(M)
    fused = M.runMPC(rom, soc0, tc, steps, cfg=cfg)
    with M.Context(rom, n, cfg) as ctx:
        assert ctx.ncon == NCON
        ctx.init_cells(soc0, tc)
        uk = np.zeros(n)
        for k in range(steps):
            v = ctx.OB_step(uk)
            zk, _, xind = ctx.iterEKF(v, uk)
            lin = ctx.EKFmatsHandler(zk, xind)
            uk, ne = ctx.iterMPC(lin, zk[:, -1])
            np.testing.assert_array_equal(v, fused["v"][k])
            np.testing.assert_array_equal(uk, fused["u"][k])
            np.testing.assert_array_equal(ne, fused["nexec"][k])


def test_wide_predmat_and_constraints(oc, M):
    rng = np.random.default_rng(5)
    n = 200
    a = np.concatenate([rng.uniform(0.3, 0.999, (n, 5)), np.ones((n, 1))], 1)
    Cr = np.concatenate([rng.normal(0, 1e-3, (n, 5)), np.zeros((n, 1))], 1)
    D = rng.normal(0, 1e-3, n)
    Phi, G = M.predMat(a, Cr, D, NP, NC)
    for i in range(0, n, 17):
        P2, G2 = oc.predmat(a[i], Cr[i], D[i], NP, NC)
        np.testing.assert_array_equal(Phi[i], P2)
        np.testing.assert_array_equal(G[i], G2)
    # constraintsMPC.m rows [Cu; -Cu; I; -I; G_v; -G_e; G_soc] from predMat's G
    lin = np.zeros((n, 35))
    lin[:, 0:6] = a
    lin[:, 11] = -1.0 / (3600 * 29.86)
    lin[:, 13:19] = Cr
    lin[:, 19] = D
    lin[:, 20:26] = Cr[::-1]
    lin[:, 26] = D[::-1]
    Mm, g = M.constraintsMPC(lin, 0.0, 0.5, 29.86, cfg=_cfg(M))
    assert Mm.shape == (n, NCON, NC) and g.shape == (n, NCON)
    for i in range(0, n, 23):
        _, Gv = oc.predmat(lin[i, 0:6], lin[i, 13:19], lin[i, 19], NP, NC)
        _, Ge = oc.predmat(lin[i, 0:6], lin[i, 20:26], lin[i, 26], NP, NC)
        np.testing.assert_array_equal(Mm[i, 4 * NC:4 * NC + NP], Gv)
        np.testing.assert_array_equal(Mm[i, 4 * NC + NP:4 * NC + 2 * NP], -Ge)
        np.testing.assert_array_equal(Mm[i, :NC], np.tril(np.ones((NC, NC))))
        np.testing.assert_array_equal(Mm[i, 2 * NC:3 * NC], np.eye(NC))


def test_wide_checkpoint_and_schedule(rom, M):
    n = 512
    soc0, tc = batch_inputs(n, seed=47)
    cfg = _cfg(M)
    with M.Context(rom, n, cfg) as a, M.Context(rom, n, cfg) as b:
        a.init_cells(soc0, tc)
        b.init_cells(soc0, tc)
        ra = a.step(70)
        rb = [b.step(k) for k in (33, 37)]
        snap = b.get_state()
        assert snap["lam"].shape == (n, NCON)
        x = b.step(10)
        b.set_state(snap)
        y = b.step(10)
    for k in ("u", "v", "soc", "phise", "nexec"):
        np.testing.assert_array_equal(ra[k], np.concatenate([r[k] for r in rb]), err_msg=k)
        np.testing.assert_array_equal(x[k], y[k], err_msg=k)


def test_wide_temperature_profile_matches_oracle(rom, oc, M):
    """Np = 20 / Nc = 10 with a temperature per step (a 10-degree ramp and a sine, per
    cell): bitwise against the C oracle over 400 closed-loop steps."""
    n, steps = 24, 400
    soc0, tc = batch_inputs(n, seed=77)
    k = np.arange(steps)[:, None]
    tc_traj = tc[None, :] + 10.0 * k / steps + 2.0 * np.sin(k / 37.0 + np.arange(n)[None, :])
    ref = oc.run(rom, soc0, tc, steps, nthreads=8, Np=NP, Nc=NC, tc_traj=tc_traj)
    out = M.runMPC(rom, soc0, tc, steps, cfg=_cfg(M), tc_traj=tc_traj)
    np.testing.assert_array_equal(out["status"], ref["status"])
    for key in ("u", "v", "soc", "phise", "nexec"):
        assert np.array_equal(out[key], ref[key], equal_nan=key != "nexec"), key


def test_wide_against_matlab_faithful_fixture(rom, M):
    """The GPU at Np = 20 / Nc = 10 against the MATLAB-faithful numpy restatement's fixtures
    (dense H, hildreth.m:28-42; tools/make_golden.py make_wide), not only against the C
    oracle: 8 batch cells x 400 steps within 1e-9 relative (north_star: 1e-6) with nexec
    exact; 4 near-limit cells at maxIter every step within 1e-9 A on u (1e-10 relative on
    v, soc, phise) and nexec exact over the first 25 steps, all 200 for the 93 % cell (test_oracle.py::
    test_c_oracle_wide_matches_numpy_fixture shows the later departure is the chaotic
    closed loop, not the method)."""
    import os
    from conftest import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "wide_batch8_400.npz"))
    out = M.runMPC(rom, g["soc0"], g["tc"], g["u"].shape[0], cfg=_cfg(M))
    np.testing.assert_array_equal(out["status"], g["status"])
    for k in ("u", "v", "soc", "phise"):
        assert _rel(out[k], g[k]).max() <= RTOL_TIGHT, k
    np.testing.assert_array_equal(out["nexec"], g["nexec"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "wide_near4_200.npz"))
    out = M.runMPC(rom, g["soc0"], g["tc"], 200, cfg=_cfg(M))
    for i in range(4):
        n = 200 if g["soc0"][i] == 93.0 else 25
        assert np.abs(out["u"][:n, i] - g["u"][:n, i]).max() <= 1e-9, i
        for k in ("v", "soc", "phise"):
            assert _rel(out[k][:n, i], g[k][:n, i]).max() <= 1e-10, (i, k)
        np.testing.assert_array_equal(out["nexec"][:n, i], g["nexec"][:n, i])
