"""GPU: initMPC's constraint switches at Np = 5 / Nc = 2 (constraintsMPC.m:15-101).

A context with a block switched off runs k_cell<P_EKF | P_LIN>, then mpcekf_switch.hip's
k_mpc_sw / k_hild_sw / k_hild_slow_sw over the enabled rows only.  Every comparison with the
C oracle (oracle_c.run, its orc_constraints / orc_hildreth on the compact stack) is bitwise.
"""
import functools
from importlib import import_module

import numpy as np
import pytest

import mexshim
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

MASKS = [(1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
TRAJ = ("u", "v", "soc", "phise", "nexec", "J_unc", "J_fin", "norm_du", "nviol")
# near-target cells (Hildreth into maxIter), then make_golden.py step 3's edge cells:
# thetae < 0 at 130 %, EKF lock-out at -15 %, 88 %
FIXED_SOC = np.array([94.9, 93.0, 85.0, 60.0, 130.0, -15.0, 88.0])
FIXED_TC = np.array([25.0, 29.0, 24.0, 35.0, 25.0, 25.0, 30.0])
MAX_HILD = 100


def ncon(mask):
    return (8 if mask[0] else 0) + (5 if mask[1] else 0) + (5 if mask[2] else 0) + 5


def cells(n):
    soc0, tc = batch_inputs(n)
    k = min(n, FIXED_SOC.size)
    soc0[:k], tc[:k] = FIXED_SOC[:k], FIXED_TC[:k]
    return soc0, tc


@pytest.fixture(scope="module")
def M():
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@functools.lru_cache(maxsize=None)
def _rom(kind):
    if kind == "nodes":
        return import_module("mpc-ekf4fastcharge_amd.rom").make_tab_rom("pchip", T_eval_degC=(25.0,))
    return import_module("mpc-ekf4fastcharge_amd").make_synth_rom(lookup=kind)


@functools.lru_cache(maxsize=None)
def _ref(mask, n, steps, kind="quintic", method="OB"):
    """The C oracle's closed loop, computed once per case and shared (read-only)."""
    import oracle_c
    oracle_c.build()
    soc0, tc = cells(n)
    ref = oracle_c.run(_rom(kind), soc0, tc, steps, nthreads=8, traj=True, constraints=mask, method=method)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _bitwise(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def _check(out, ref, what):
    for k in TRAJ:
        _bitwise(out[k], ref[k], f"{what} {k}")
    _bitwise(out["status"], ref["status"], f"{what} status")


def _run(M, mask, n, steps, kind="quintic", method="OB", **kw):
    soc0, tc = cells(n)
    with M.Context(_rom(kind), n, M.make_config(constraints=mask, method=method)) as ctx:
        assert ctx.ncon == ncon(mask)
        ctx.init_cells(soc0, tc)
        out = ctx.step(steps, outputs=TRAJ, **kw)
        st = ctx.get_state()
    out["status"], out["lam"] = st["status"], st["lam"]
    return out


CASES = [(m, 65, "quintic", "OB") for m in MASKS] + \
        [(m, n, "quintic", "OB") for m in ((1, 1, 0), (0, 0, 0)) for n in (1, 3, 257)] + \
        [((1, 1, 0), 65, "quintic", "MB"), ((1, 1, 0), 65, "linear", "OB"), ((1, 1, 0), 65, "nodes", "OB")]


@pytest.mark.parametrize("mask,n,kind,method", CASES)
def test_fused_loop_matches_oracle(M, mask, n, kind, method):
    """u, v, soc, phise, nexec, the cost log and status over 300 fused steps: the oracle's bits."""
    steps = 300
    ref = _ref(mask, n, steps, kind, method)
    # not vacuous: hildreth.m runs, and runs into maxIter, on some cell
    assert (ref["nexec"] > 0).any() and (ref["nexec"] == MAX_HILD).any()
    out = _run(M, mask, n, steps, kind, method)
    _check(out, ref, f"{mask} n={n} {kind} {method}")
    assert out["lam"].shape == (n, ncon(mask))
    assert (out["lam"] >= 0).all() or np.isnan(out["lam"]).any()


def test_switched_off_constraint_changes_the_run(M):
    """(1,1,0) is not (1,1,1): the oracle's trajectories differ, so the cases above could not
    pass on the all-on kernels."""
    a, b = _ref((1, 1, 0), 65, 300), _ref((1, 1, 1), 65, 300)
    assert not np.array_equal(a["u"], b["u"], equal_nan=True)


def test_all_on_guard(M):
    """A context created with switches (1,1,1) is the default-config context, bit for bit."""
    n, steps = 65, 120
    soc0, tc = cells(n)
    rom = _rom("quintic")
    with M.Context(rom, n) as d, M.Context(rom, n, M.make_config(constraints=(1, 1, 1))) as e:
        assert d.ncon == 23 and e.ncon == 23
        outs = []
        for c in (d, e):
            c.init_cells(soc0, tc)
            o = c.step(steps, outputs=TRAJ)
            st = c.get_state()
            o["status"], o["lam"] = st["status"], st["lam"]
            outs.append(o)
    for k in TRAJ + ("status", "lam"):
        _bitwise(outs[0][k], outs[1][k], k)


@pytest.mark.parametrize("mask", [(1, 1, 0), (0, 0, 1)])
def test_solver_cross_check(M, mask):
    """The masked fused solver against the generic mpcekf_hildreth (k_hildreth_any) on the same
    problem: compact M / gamma from mpcekf_constraints, E / F from the step's problem record,
    the warm start from get_state.  lambda, DU (through u) and nexec agree bitwise."""
    n, pre = 65, 40
    soc0, tc = cells(n)
    rom = _rom("quintic")
    cfg = M.make_config(constraints=mask)
    nc = ncon(mask)
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.step(pre)
        hit = 0
        for k in range(12):
            st0 = ctx.get_state()
            uk_1 = st0["scal"][:, ctx.SCALARS.index("uk_1")].copy()
            # the step by stages, so that its linearisation record is in hand
            v = ctx.OB_step(st0["scal"][:, ctx.SCALARS.index("uk")].copy())
            zk, _, xi = ctx.iterEKF(v, st0["scal"][:, ctx.SCALARS.index("uk")].copy())
            lin = ctx.EKFmatsHandler(zk, xi)
            uk, ne = ctx.iterMPC(lin, zk[:, -1])
            prob, hflag = ctx.get_hild_problems()
            lam1 = ctx.get_state()["lam"]
            ok = (hflag != 0) & np.isfinite(lin).all(axis=1)
            if not ok.any():
                continue
            Mm, g = M.constraintsMPC(lin[ok], uk_1[ok], zk[ok, -1], rom.Q, cfg)
            assert Mm.shape == (int(ok.sum()), nc, 2) and g.shape == (int(ok.sum()), nc)
            E = prob[0:4, ok].T.reshape(-1, 2, 2).copy()
            F = prob[4:6, ok].T.copy()
            DU, lam, nex = M.hildreth(E, F, Mm, g, lambda0=st0["lam"][ok], maxIter=MAX_HILD, tol=cfg.hild_tol)
            _bitwise(lam, lam1[ok], f"{mask} step {k} lambda")
            _bitwise(nex, ne[ok], f"{mask} step {k} nexec")
            _bitwise(DU[:, 0] + uk_1[ok], uk[ok], f"{mask} step {k} uk")
            # a disabled block's record fields read 0
            if not mask[1]:
                assert (prob[6:11, ok] == 0).all() and (prob[21 + 8:21 + 13, ok] == 0).all()
            if not mask[2]:
                assert (prob[11:16, ok] == 0).all() and (prob[21 + 13:21 + 18, ok] == 0).all()
            if not mask[0]:
                assert (prob[21:21 + 8, ok] == 0).all()
            hit += int(ok.sum())
        assert hit > 0


def test_call_splitting_graph_and_device_outputs(M):
    """(1,1,0): one call of 64 steps = 64 calls of one step = the same under graph replay =
    outputs_on_device, bitwise."""
    mask, n, steps = (1, 1, 0), 65, 64
    soc0, tc = cells(n)
    rom = _rom("quintic")
    cfg = M.make_config(constraints=mask)
    keys = ("u", "v", "soc", "phise", "nexec")
    one = _run(M, mask, n, steps)
    for graph in (False, True):
        with M.Context(rom, n, cfg) as ctx:
            ctx.init_cells(soc0, tc)
            ctx.set_graph(graph)
            parts = [ctx.step(1, outputs=keys) for _ in range(steps)]
            lam = ctx.get_state()["lam"]
        for k in keys:
            _bitwise(np.concatenate([p[k] for p in parts]), one[k], f"graph={graph} {k}")
        _bitwise(lam, one["lam"], f"graph={graph} lambda")
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc)
        bufs = {k: M.DeviceBuffer((steps, n), np.int32 if k == "nexec" else np.float64) for k in keys}
        ctx.step_device(steps, **bufs)
        ctx.sync()
        for k in keys:
            _bitwise(bufs[k].to_host(), one[k], f"device outputs {k}")
            bufs[k].free()
        _bitwise(ctx.get_state()["lam"], one["lam"], "device outputs lambda")


@pytest.mark.parametrize("n", [9000, 1024])
def test_both_batch_size_mappings(M, n):
    """A batch above and one below the small-batch threshold (8,192 cells): a switched context
    takes the k_cell route at either size, and matches the oracle."""
    mask, steps = (1, 1, 0), 40
    _check(_run(M, mask, n, steps), _ref(mask, n, steps), f"n={n}")


def test_timing_buckets(M):
    """mpcekf_set_timing on a switched context: results unchanged, the MPC kernel counted in
    'cell' and the Hildreth pair in 'hild'."""
    mask, n, steps = (1, 1, 0), 65, 30
    soc0, tc = cells(n)
    with M.Context(_rom("quintic"), n, M.make_config(constraints=mask)) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_timing(True)
        out = ctx.step(steps, outputs=TRAJ)
        t = ctx.get_timing()
    ref = _ref(mask, n, 300)
    for k in TRAJ:
        _bitwise(out[k], ref[k][:steps], k)
    assert t["cell"][1] == steps and t["hild"][1] == steps and t["cell"][0] > 0 and t["hild"][0] > 0


@pytest.mark.parametrize("asynchronous", [False, True])
def test_stage_route(M, oc, asynchronous):
    """(1,1,0): plant -> ekf -> linearize -> mpc_step_ex with the device hand-offs, synchronous
    and _async, over 60 steps equals the fused step; each step's lambda is the C oracle's
    iterMPC (orc_mpc_lin) on the compact warm start."""
    mask, n, steps = (1, 1, 0), 65, 60
    soc0, tc = cells(n)
    rom = _rom("quintic")
    fused = _run(M, mask, n, steps)
    with M.Context(rom, n, M.make_config(constraints=mask)) as ctx:
        ctx.init_cells(soc0, tc)
        u = np.zeros(n)
        for k in range(steps):
            st0 = ctx.get_state() if k % 10 == 9 else None
            ctx.asynchronous = asynchronous
            v = ctx.OB_step(u, tc)
            zk, _, _ = ctx.iterEKF(None if asynchronous else v, u, tc, xind=False)
            lin = ctx.EKFmatsHandler(None, None, tc, keep=not (st0 is not None and not asynchronous))
            ctx.asynchronous = False
            u, ne, cost = ctx.iterMPC(None, None, cost=True)   # synchronous: completes the step
            _bitwise(u, fused["u"][k], f"step {k} u")
            _bitwise(ne, fused["nexec"][k], f"step {k} nexec")
            _bitwise(cost["J_final"], fused["J_fin"][k], f"step {k} J_fin")
            _bitwise(cost["viol"], fused["nviol"][k], f"step {k} nviol")
            if st0 is not None and not asynchronous:
                ok = np.isfinite(lin).all(axis=1) & (st0["status"] == 0)
                uk_1 = st0["scal"][:, ctx.SCALARS.index("uk_1")]
                ru, rn, _, rl = oc.mpc_lin(rom, lin[ok], zk[ok, -1], uk_1[ok], st0["lam"][ok], constraints=mask)
                _bitwise(u[ok], ru, f"step {k} oracle u")
                _bitwise(ne[ok], rn, f"step {k} oracle nexec")
                _bitwise(ctx.get_state()["lam"][ok], rl, f"step {k} oracle lambda")
        _bitwise(ctx.get_state()["lam"], fused["lam"], "final lambda")


def test_stage_route_through_mex_gateway(M):
    """The drop-ins' command sequence through the MEX gateway on a (1,1,0) handle."""
    mexshim.build()
    mask, n, steps = (1, 1, 0), 65, 20
    soc0, tc = cells(n)
    rom = _rom("quintic")
    fused = _run(M, mask, n, steps)
    e = np.zeros((0, 0))
    h = mexshim.mex("create", mexshim.rom_struct(rom), {"use_eta": 0.0}, 0.0, float(n))
    try:
        mexshim.mex("init", h, soc0, tc, nargout=0)
        uk = np.zeros((1, n))
        tk = tc[None, :].copy()
        for k in range(steps):
            v = mexshim.mex("plant", h, uk, tk)
            zk, _ = mexshim.mex("ekf", h, v, uk, tk, nargout=2)
            mexshim.mex("linearize", h, e, e, e, tk)
            uk = mexshim.mex("mpc", h, e, zk[-1:, :], nargout=6)[0]
            _bitwise(uk.ravel(), fused["u"][k], f"step {k}")
    finally:
        mexshim.mex("destroy", h, nargout=0)


def test_state_round_trip(M):
    """(1,0,0): get_state -> new context -> set_state -> continue equals the uninterrupted
    run; lambda is [n, 13] in the reference's row order."""
    mask, n, a, b = (1, 0, 0), 65, 150, 150
    soc0, tc = cells(n)
    rom = _rom("quintic")
    cfg = M.make_config(constraints=mask)
    whole = _run(M, mask, n, a + b)
    with M.Context(rom, n, cfg) as c1:
        c1.init_cells(soc0, tc)
        c1.step(a)
        st = c1.get_state()
    assert st["lam"].shape == (n, 13)
    assert (st["lam"] != 0).any()
    with M.Context(rom, n, cfg) as c2:
        c2.init_cells(soc0, tc)
        c2.set_state(st)
        out = c2.step(b, outputs=TRAJ)
        lam = c2.get_state()["lam"]
    for k in TRAJ:
        _bitwise(out[k], whole[k][a:], k)
    _bitwise(lam, whole["lam"], "lambda")


def test_obs_negphise0_with_and_without_eta(M):
    """The README's figure pair: without the eta constraint the plant's negPhise0 falls below
    phise_min on some cell; with it, it stays within 1e-3 of the limit."""
    n, steps = 65, 300
    soc0, tc = cells(n)
    live = (soc0 > 0) & (soc0 < 100)
    rom = _rom("quintic")
    lo = {}
    for mask in ((1, 1, 1), (1, 1, 0)):
        cfg = M.make_config(constraints=mask)
        with M.Context(rom, n, cfg) as ctx:
            ctx.init_cells(soc0, tc)
            out = ctx.step(steps, obs=("negPhise0",))
        p = out["obs"]["negPhise0"]
        assert p.shape == (steps, n)
        lo[mask] = np.nanmin(p[:, live], axis=0)
        phise_min = cfg.phise_min
    assert (lo[(1, 1, 0)] < phise_min).any()
    assert not (lo[(1, 1, 1)] < phise_min - 1e-3).any()


def test_wide_horizon_refuses_a_switch(M):
    """Np = 20 / Nc = 10 with use_eta = 0: MPCEKF_E_UNSUPPORTED, and the message names the horizon."""
    with pytest.raises(M.MpcekfError) as ei:
        M.Context(_rom("quintic"), 4, M.make_config(Np=20, Nc=10, constraints=(1, 1, 0)))
    assert "mpcekf error -4:" in str(ei.value)   # MPCEKF_E_UNSUPPORTED
    assert "Np=20" in str(ei.value) and "Nc=10" in str(ei.value)
