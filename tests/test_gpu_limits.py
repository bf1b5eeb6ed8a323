"""GPU: per-cell MPC limits and targets across a batch (mpcekf_set_limits; runMPC.m:30-44 per cell).

A context with per-cell limits runs k_cell<P_EKF | P_LIN>, then k_mpc_pc<SW> (k_mpc_wide_pc at
Np = 20 / Nc = 10) with the cell's own eight limit values, then the Hildreth kernels of its
constraint mask.  The reference is the C oracle run once per group of cells with that group's
scalars (limit_groups.py; cell c is in group c % G, so every wave mixes groups).  Every
comparison is bitwise (NaN = NaN).
"""
from importlib import import_module

import numpy as np
import pytest

import limit_groups as lg
import mexshim
from limit_groups import G, GROUPS, TRAJ, bitwise

pytestmark = pytest.mark.gpu

MASKS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
MAX_HILD = 100
HORIZONS = {5: dict(Np=5, Nc=2), 20: dict(Np=20, Nc=10)}


@pytest.fixture(scope="module")
def M():
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


def _cfg(M, Np=5, mask=(1, 1, 1), method="OB", **kw):
    return M.make_config(constraints=mask, method=method, **HORIZONS[Np], **kw)


def _run(M, n, steps, cfg, limits=None, outputs=TRAJ):
    soc0, tc = lg.inputs(n)
    with M.Context(lg._rom("quintic"), n, cfg) as ctx:
        ctx.init_cells(soc0, tc)
        if limits:
            ctx.set_limits(**limits)
        out = ctx.step(steps, outputs=outputs)
        st = ctx.get_state()
    out["status"], out["lam"] = st["status"], st["lam"]
    return out


def _check(out, ref, what):
    for k in TRAJ:
        bitwise(out[k], ref[k], f"{what} {k}")
    bitwise(out["status"], ref["status"], f"{what} status")


# ---- 1. uniform arrays change nothing ------------------------------------------------------
@pytest.mark.parametrize("Np,n,steps", [(5, 193, 120), (20, 70, 60)])
def test_uniform_arrays_change_nothing(M, Np, n, steps):
    """All nine fields set to arrays constant at the configuration's values: the split route
    with per-cell loads gives the bits of the default context (fused k_cell at Np = 5), with no
    oracle in between: u, v, soc, phise, nexec, the cost log, status and lambda."""
    cfg = _cfg(M, Np)
    a = _run(M, n, steps, cfg)
    b = _run(M, n, steps, cfg, limits=lg.uniform_arrays(n))
    for k in TRAJ + ("status", "lam"):
        bitwise(b[k], a[k], f"Np={Np} {k}")
    assert (a["nexec"] > 0).any()


# ---- 2. heterogeneous batch against the oracle ---------------------------------------------
def _floors(Np, n, steps, mask):
    """Asserted on the oracle alone, before the GPU is compared.  Returns the per-group reference.

    (a) Every group whose changed field enters the problem under this mask differs from the
        default-limits run in at least one bit on its own cells.  A field of a switched-off block
        (v_max without useVoltage, ...) cannot: such a group must equal the default run instead.
    (b) Over the batch hildreth.m runs, and runs into maxIter.
    (c) At least three quarters of the cells end with status 0 -- under every mask but (0,0,0):
        there the reference's own default run loses 154 of these 193 cells within 30 steps
        (nothing bounds the current; thetae < 0), the groups whose fields are all switched off
        are that run, and no choice of limits changes it.  Status still has to match bit for bit.
    """
    ref = lg.oracle_groups("quintic", n, steps, mask=mask, **HORIZONS[Np])
    base = lg.oracle_default("quintic", n, steps, mask=mask, **HORIZONS[Np])
    d = lg.differs(ref, base)
    g = lg.group_of(n)
    for j, grp in enumerate(GROUPS):
        if lg.active(grp, mask):
            assert d[g == j].any(), f"group {j} {grp} equals the default run under {mask}"
        else:
            assert not d[g == j].any(), f"group {j} {grp} has no enabled row under {mask} but differs"
    assert (ref["nexec"] > 0).any() and (ref["nexec"] == MAX_HILD).any()
    if mask != (0, 0, 0):
        assert (ref["status"] == 0).mean() >= 0.75, f"{mask}: {(ref['status'] != 0).sum()} of {n} cells in error"
    return ref


def test_oracle_floors_ztol():
    """The several-fields group without its z_tol is another run: z_tol is not a passenger."""
    n, steps = 193, 400
    soc0, tc = lg.inputs(n)
    idx = np.flatnonzero(lg.group_of(n) == G - 1)
    grp = dict(GROUPS[-1], z_tol=0.0)
    o = lg.oracle_c.run(lg._rom("quintic"), soc0[idx], tc[idx], steps, nthreads=8, **grp)
    ref = lg.oracle_groups("quintic", n, steps)
    assert not np.array_equal(o["u"], ref["u"][:, idx], equal_nan=True)


@pytest.mark.parametrize("mask", MASKS)
def test_heterogeneous_batch_np5(M, mask):
    """Np = 5, every constraint mask: 193 cells in 9 groups over 400 steps, the oracle's bits."""
    n, steps = 193, 400
    ref = _floors(5, n, steps, mask)
    out = _run(M, n, steps, _cfg(M, 5, mask), limits=lg.limit_arrays(n))
    _check(out, ref, f"{mask}")


def test_heterogeneous_batch_np20(M):
    """Np = 20 / Nc = 10, all switches on: 70 cells in 9 groups over 200 steps."""
    n, steps = 70, 200
    ref = _floors(20, n, steps, (1, 1, 1))
    out = _run(M, n, steps, _cfg(M, 20), limits=lg.limit_arrays(n))
    _check(out, ref, "Np=20")


# ---- 3. the large-batch mapping -------------------------------------------------------------
def test_large_batch(M):
    """9,000 cells (above the 8,192-cell threshold; spread_block's full blocks), 60 steps, G = 3:
    the Crate, target and du_max groups, which differ from the defaults from step 0."""
    n, steps, sel = 9000, 60, (2, 3, 4)
    ref = lg.oracle_groups("quintic", n, steps, sel=sel)
    base = lg.oracle_default("quintic", n, steps)
    d, g = lg.differs(ref, base), lg.group_of(n, lg.pick(sel))
    assert all(d[g == j].all() for j in range(len(sel)))
    out = _run(M, n, steps, _cfg(M), limits=lg.limit_arrays(n, lg.pick(sel)))
    _check(out, ref, "n=9000")


# ---- 4. the MB filter -----------------------------------------------------------------------
def test_model_blend_filter(M):
    n, steps = 65, 120
    ref = lg.oracle_groups("quintic", n, steps, method="MB")
    base = lg.oracle_default("quintic", n, steps, method="MB")
    assert lg.differs(ref, base).any() and (ref["nexec"] > 0).any()
    out = _run(M, n, steps, _cfg(M, method="MB"), limits=lg.limit_arrays(n))
    _check(out, ref, "MB")


# ---- 5. the stage route ---------------------------------------------------------------------
@pytest.mark.parametrize("Np,n", [(5, 65), (20, 35)])
def test_stage_route(M, oc, Np, n):
    """OB_step -> iterEKF -> EKFmatsHandler(keep) -> iterMPC(None, ..) on a per-cell context
    equals the fused step of a twin; one step's iterMPC equals orc_mpc_lin per group; mpc_diag
    of the group-g cells equals a uniform context's, configured with group g's scalars, on
    the same records."""
    steps, probe = 30, 12
    soc0, tc = lg.inputs(n)
    rom = lg._rom("quintic")
    lim = lg.limit_arrays(n)
    g = lg.group_of(n)
    fused = _run(M, n, steps, _cfg(M, Np), limits=lim)
    with M.Context(rom, n, _cfg(M, Np)) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_limits(**lim)
        u = np.zeros(n)
        for k in range(steps):
            st0 = ctx.get_state() if k == probe else None
            v = ctx.OB_step(u, tc)
            zk, _, _ = ctx.iterEKF(v, u, tc, xind=False)
            lin = ctx.EKFmatsHandler(None, None, tc, keep=st0 is None)
            if st0 is not None:
                uk_1 = st0["scal"][:, ctx.SCALARS.index("uk_1")].copy()
                poles, sv = ctx.mpc_diag(None)
                poles, sv = poles.copy(), sv.copy()
            u, ne, cost = ctx.iterMPC(None, None, cost=True)
            bitwise(u, fused["u"][k], f"step {k} u")
            bitwise(ne, fused["nexec"][k], f"step {k} nexec")
            bitwise(cost["J_uncon"], fused["J_unc"][k], f"step {k} J_unc")
            bitwise(cost["J_final"], fused["J_fin"][k], f"step {k} J_fin")
            bitwise(cost["norm_DU"], fused["norm_du"][k], f"step {k} norm_du")
            bitwise(cost["viol"], fused["nviol"][k], f"step {k} nviol")
            if st0 is not None:
                lam1 = ctx.get_state()["lam"]
                assert np.isfinite(lin).all() and (st0["status"] == 0).all()
                for j, grp in enumerate(GROUPS):
                    idx = np.flatnonzero(g == j)
                    ru, rn, _, rl = oc.mpc_lin(rom, lin[idx], zk[idx, -1], uk_1[idx], st0["lam"][idx],
                                               **HORIZONS[Np], **grp)
                    bitwise(u[idx], ru, f"group {j} oracle u")
                    bitwise(ne[idx], rn, f"group {j} oracle nexec")
                    bitwise(lam1[idx], rl, f"group {j} oracle lambda")
                # Ru reads du_max and F reads the target: groups 3 (target), 4 (du_max), 8 (several)
                for j in (3, 4, G - 1):
                    idx = np.flatnonzero(g == j)
                    with M.Context(rom, n, _cfg(M, Np, **lg.config_kwargs(GROUPS[j]))) as uni:
                        uni.init_cells(soc0, tc)
                        up, us = uni.mpc_diag(lin, uk_1)
                    bitwise(poles[idx].view(np.float64), up[idx].copy().view(np.float64), f"group {j} poles")
                    bitwise(sv[idx], us[idx], f"group {j} sv")
                with M.Context(rom, n, _cfg(M, Np)) as uni:   # and they are not the default context's
                    uni.init_cells(soc0, tc)
                    up, _ = uni.mpc_diag(lin, uk_1)
                idx = np.flatnonzero(g == 4)
                assert not np.array_equal(poles[idx], up[idx], equal_nan=True)
        bitwise(ctx.get_state()["lam"], fused["lam"], "final lambda")


# ---- 6. / 7. mid-charge change, clear -------------------------------------------------------
CFG2 = dict(target_soc=80.0, Crate=3.0, u_max=-1.0, du_min=-20.0, du_max=20.0, v_max=3.95, phise_min=0.10,
            z_max=0.60, z_tol=0.01)


def _transplant(M, n, a, b, cfg_a, lim_a, cfg_b):
    """cfg_a (+ lim_a) for a steps; its get_state loaded into a fresh context under cfg_b; b steps."""
    soc0, tc = lg.inputs(n)
    rom = lg._rom("quintic")
    with M.Context(rom, n, cfg_a) as c1:
        c1.init_cells(soc0, tc)
        if lim_a:
            c1.set_limits(**lim_a)
        c1.step(a)
        st = c1.get_state()
    with M.Context(rom, n, cfg_b) as c2:
        c2.init_cells(soc0, tc)
        c2.set_state(st)
        out = c2.step(b, outputs=TRAJ)
        out["lam"] = c2.get_state()["lam"]
    return out


@pytest.mark.parametrize("Np,n", [(5, 65), (20, 35)])
def test_mid_charge_change(M, Np, n):
    """50 steps under cfg1, set_limits to cfg2's values for every cell, 50 more: the second half
    equals a context created under cfg2 from the checkpoint after the first."""
    a = b = 50
    soc0, tc = lg.inputs(n)
    with M.Context(lg._rom("quintic"), n, _cfg(M, Np)) as ctx:
        ctx.init_cells(soc0, tc)
        first = ctx.step(a, outputs=TRAJ)
        ctx.set_limits(**CFG2)
        out = ctx.step(b, outputs=TRAJ)
        out["lam"] = ctx.get_state()["lam"]
    ref = _transplant(M, n, a, b, _cfg(M, Np), None, _cfg(M, Np, **CFG2))
    for k in TRAJ + ("lam",):
        bitwise(out[k], ref[k], f"Np={Np} {k}")
    whole = _run(M, n, a + b, _cfg(M, Np))
    for k in TRAJ:
        bitwise(first[k], whole[k][:a], f"first half {k}")
    assert not np.array_equal(out["u"], whole["u"][a:], equal_nan=True)   # the change changed the run


def test_clear(M):
    """30 steps per-cell, clear_limits, 30 steps: the second half equals a default context
    continued from the checkpoint after the first."""
    n, a, b = 65, 30, 30
    soc0, tc = lg.inputs(n)
    lim = lg.limit_arrays(n)
    with M.Context(lg._rom("quintic"), n, _cfg(M)) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_limits(**lim)
        first = ctx.step(a, outputs=TRAJ)
        ctx.clear_limits()
        out = ctx.step(b, outputs=TRAJ)
        out["lam"] = ctx.get_state()["lam"]
        for k, v in ctx.get_limits().items():
            assert (v == getattr(ctx.cfg, k)).all(), k
    ref = _transplant(M, n, a, b, _cfg(M), lim, _cfg(M))
    for k in TRAJ + ("lam",):
        bitwise(out[k], ref[k], k)
    bitwise(first["u"], lg.oracle_groups("quintic", n, a)["u"], "first half u")


# ---- 8. get ---------------------------------------------------------------------------------
def test_get_limits(M):
    n = 21
    soc0, tc = lg.inputs(n)
    cfg = _cfg(M, v_max=4.05)
    with M.Context(lg._rom("quintic"), n, cfg) as ctx:
        for k, v in ctx.get_limits().items():             # never set: the configuration's scalars, before init_cells too
            assert v.shape == (n,) and (v == getattr(cfg, k)).all(), k
        ctx.init_cells(soc0, tc)
        ph, du = np.linspace(0.05, 0.12, n), -np.arange(1.0, n + 1)
        ctx.set_limits(phise_min=ph, du_max=du)           # a negative du_max is legitimate
        ctx.set_limits(Crate=1.5)                         # a later call keeps the earlier fields
        got = ctx.get_limits()
        bitwise(got["phise_min"], ph, "phise_min")
        bitwise(got["du_max"], du, "du_max")
        assert (got["Crate"] == 1.5).all()
        for k in ("target_soc", "u_max", "du_min", "v_max", "z_max", "z_tol"):
            assert (got[k] == getattr(cfg, k)).all(), k
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: set_limits: fields"):
            ids = np.array([0, 9], dtype=np.int32)
            M.check(ctx.L.mpcekf_set_limits(ctx.h, 2, M.iptr(ids), M.dptr(np.zeros((2, n)))))
        with pytest.raises(M.MpcekfError, match="given twice"):
            ids = np.array([3, 3], dtype=np.int32)
            M.check(ctx.L.mpcekf_get_limits(ctx.h, 2, M.iptr(ids), M.dptr(np.zeros((2, n)))))
        with pytest.raises(M.MpcekfError, match="nfields = 10 outside 1..9"):
            ids = np.arange(10, dtype=np.int32)
            M.check(ctx.L.mpcekf_set_limits(ctx.h, 10, M.iptr(ids), M.dptr(np.zeros((10, n)))))
        with pytest.raises(M.MpcekfError, match="set_limits: null values"):
            M.check(ctx.L.mpcekf_set_limits(ctx.h, 1, M.iptr(np.zeros(1, np.int32)), None))
        with pytest.raises(M.MpcekfError, match="get_limits: null fields"):
            M.check(ctx.L.mpcekf_get_limits(ctx.h, 1, None, M.dptr(np.zeros((1, n)))))
        bitwise(ctx.get_limits()["phise_min"], ph, "a refused call changes nothing")


def test_run_mpc_limits_keyword(M):
    """runMPC(..., limits=dict) is set_limits after init_cells and before the first step."""
    n, steps = 65, 40
    soc0, tc = lg.inputs(n)
    out = M.runMPC(lg._rom("quintic"), soc0, tc, steps, limits=lg.limit_arrays(n))
    ref = lg.oracle_groups("quintic", n, steps)
    for k in ("u", "v", "soc", "phise", "nexec", "status"):
        bitwise(out[k], ref[k], k)


# ---- 9. graph replay ------------------------------------------------------------------------
def test_graph_replay_across_set_and_clear(M):
    """set_graph(True): 20 one-step calls, set_limits, 20 more, a second set_limits (the same
    buffer, no new capture needed), 10 more, clear_limits, 10 more -- the same sequence without
    graph replay, bitwise."""
    n = 65
    soc0, tc = lg.inputs(n)
    keys = ("u", "v", "soc", "phise", "nexec")
    lim = lg.limit_arrays(n)
    runs = []
    for graph in (False, True):
        with M.Context(lg._rom("quintic"), n, _cfg(M)) as ctx:
            ctx.init_cells(soc0, tc)
            ctx.set_graph(graph)
            parts = [ctx.step(1, outputs=keys) for _ in range(20)]
            ctx.set_limits(**lim)
            parts += [ctx.step(1, outputs=keys) for _ in range(20)]
            ctx.set_limits(**CFG2)
            parts += [ctx.step(1, outputs=keys) for _ in range(10)]
            ctx.clear_limits()
            parts += [ctx.step(1, outputs=keys) for _ in range(10)]
            out = {k: np.concatenate([p[k] for p in parts]) for k in keys}
            out["lam"] = ctx.get_state()["lam"]
        runs.append(out)
    for k in keys + ("lam",):
        bitwise(runs[1][k], runs[0][k], f"graph {k}")
    # and the first 40 steps are the known runs
    bitwise(runs[0]["u"][:20], lg.oracle_default("quintic", n, 20)["u"], "first 20 steps")
    assert not np.array_equal(runs[0]["u"][20:40], _run(M, n, 40, _cfg(M))["u"][20:], equal_nan=True)


def test_timing_buckets(M):
    """mpcekf_set_timing on a per-cell context: k_mpc_pc counted in 'cell', the Hildreth pair in
    'hild', results unchanged."""
    n, steps = 65, 30
    soc0, tc = lg.inputs(n)
    with M.Context(lg._rom("quintic"), n, _cfg(M)) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_limits(**lg.limit_arrays(n))
        ctx.set_timing(True)
        out = ctx.step(steps, outputs=TRAJ)
        t = ctx.get_timing()
    ref = lg.oracle_groups("quintic", n, steps)
    for k in TRAJ:
        bitwise(out[k], ref[k], k)
    assert t["cell"][1] == steps and t["hild"][1] == steps and t["cell"][0] > 0 and t["hild"][0] > 0


# ---- 10. the MEX gateway --------------------------------------------------------------------
def test_mex_gateway(M):
    """'setlimits' / 'getlimits' round trip, a fused 'step' after 'setlimits' gives the ctypes
    path's bits, and 'clearlimits' returns the cfg scalars."""
    mexshim.build()
    n, steps = 16, 20
    soc0, tc = lg.inputs(n)
    rom = lg._rom("quintic")
    lim = lg.limit_arrays(n)
    ref = _run(M, n, steps, _cfg(M), limits=lim, outputs=("u", "v", "soc", "phise", "nexec"))
    idx = np.array([[7.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.0]])             # 1-based, any order
    vals = np.stack([lim[M.Context.LIMIT_FIELDS[int(i) - 1]] for i in idx[0]], axis=1)   # ncells x 9
    h = mexshim.mex("create", mexshim.rom_struct(rom), {}, 0.0, float(n))
    try:
        mexshim.mex("init", h, soc0, tc, nargout=0)
        mexshim.mex("setlimits", h, idx, vals, nargout=0)
        bitwise(mexshim.mex("getlimits", h, idx), vals, "getlimits")
        bitwise(mexshim.mex("getlimits", h, np.array([[6.0]])), lim["v_max"][:, None], "getlimits v_max")
        u, v, soc, phise, nexec = mexshim.mex("step", h, float(steps), nargout=5)
        for k, a in (("u", u), ("v", v), ("soc", soc), ("phise", phise), ("nexec", nexec)):
            bitwise(a.T, ref[k], f"mex {k}")
        with pytest.raises(mexshim.MexError, match=r"mpcekf:arg: setlimits: values \(ncells x numel\(idx\)\)"):
            mexshim.mex("setlimits", h, idx, vals[:, :8].copy(), nargout=0)
        mexshim.mex("clearlimits", h, nargout=0)
        assert (mexshim.mex("getlimits", h, np.array([[6.0]])) == M.make_config().v_max).all()
    finally:
        mexshim.mex("destroy", h, nargout=0)
