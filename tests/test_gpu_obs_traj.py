"""GPU: the plant's observables along the fused closed loop (mpcekf_step_ex_obs, k_obs_traj,
Context.step(obs=...), runMPC(obs=...), step_device(obs=...), the gateway's 'stepobs').

References: tests/obs_ref.ob_obs on the state read back before each one-step call
(tolerance 1e-12 * max(1, max|field|), the bound tests/test_gpu_obs.py uses for it), and
the library against itself, bit for bit: one call against split calls (the lazy replay),
flush schedules, every kernel that can run the plant, the stage route's record, graph
replay, device outputs.  Shapes n = 1, 3, 65, 257: a partial quad / wave, a wave boundary
(16 cells a wave), a block boundary (128 cells a block).
"""
import ctypes as C

import numpy as np
import pytest

import mexshim
import obs_ref
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

KEYS = ("u", "v", "soc", "phise")
ST_ERROR = 1
E_ARG = -1


@pytest.fixture(scope="module")
def M(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def R(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.rom")


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ in bits"


def _obs_equal(a, b, what):
    assert tuple(a) == tuple(b), (what, tuple(a), tuple(b))
    for f in a:
        _bits_equal(a[f], b[f], f"{what}: {f}")


def _ref_step(rom, st, soc0n, soc0p, tc):
    """ob_obs on every cell of a get_state() snapshot, with the command the next fused step
    applies (scal[:, MPCEKF_S_UK]): {field: [n] or [n, len]}."""
    n = st["scal"].shape[0]
    per = [obs_ref.ob_obs(rom, st["bigX"][c], st["scal"][c, 0], st["scal"][c, 1], soc0n[c], soc0p[c],
                          st["scal"][c, 6], tc[c]) for c in range(n)]
    return {k: np.array([p[k] for p in per]).reshape((n,) if np.ndim(per[0][k]) == 0 else (n, np.size(per[0][k])))
            for k in obs_ref.OBS_FIELDS}


def _split(M, rom, n, soc0, tc0, steps, cfg=None, tc=None, obs=True, ref=False, tol=1e-12):
    """`steps` calls of step(1, obs=...): the trajectories stacked; every model is current
    between calls.  ref: each call's obs also against ob_obs on the state before it."""
    rows = []
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc0)
        st0 = ctx.get_state()
        soc0n, soc0p = st0["scal"][:, 0].copy(), st0["scal"][:, 1].copy()   # SOC0n/p: the initial averages
        for k in range(steps):
            st = ctx.get_state() if ref else None
            tk = None if tc is None else tc[k:k + 1]
            o = ctx.step(1, tc=tk, obs=obs)
            rows.append(o)
            if not ref:
                continue
            r = _ref_step(rom, st, soc0n, soc0p, np.broadcast_to(tc0 if tc is None else tc[k], (n,)))
            assert tuple(o["obs"]) == obs_ref.OBS_FIELDS
            for f in obs_ref.OBS_FIELDS:
                got = o["obs"][f][0]
                assert got.shape == r[f].shape, (f, got.shape, r[f].shape)
                if not r[f].size:
                    continue
                err = float(np.max(np.abs(got - r[f])))
                atol = tol * max(1.0, float(np.max(np.abs(r[f]))))
                print(f"n={n} step {k} {f}: max err {err:.3g} (atol {atol:.3g})")
                assert err <= atol, (f, k, err, atol)
    out = {k: np.concatenate([r[k] for r in rows]) for k in KEYS + ("nexec",)}
    out["obs"] = {f: np.concatenate([r["obs"][f] for r in rows]) for f in rows[0]["obs"]}
    return out


def _single(M, rom, n, soc0, tc0, steps, cfg=None, tc=None, obs=True, **kw):
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc0)
        return ctx.step(steps, tc=tc, obs=obs, **kw)


def _same_run(a, b, what):
    for k in KEYS:
        _bits_equal(a[k], b[k], f"{what}: {k}")
    assert np.array_equal(a["nexec"], b["nexec"]), what
    _obs_equal(a["obs"], b["obs"], what)


# ---- 1. against the numpy reference ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("lookup", ["linear", "quintic"])
def test_obs_traj_matches_reference(P, M, lookup, n):
    soc0, tc = batch_inputs(n, seed=211 + n)
    _split(M, P.make_synth_rom(lookup=lookup), n, soc0, tc, 12, ref=True)


@pytest.mark.parametrize("n", [3, 65])
def test_obs_traj_matches_reference_node_tables(M, R, n):
    soc0, tc = batch_inputs(n, seed=223 + n)
    _split(M, R.make_tab_rom("linear", T_eval_degC=(25.0,)), n, soc0, tc, 12, ref=True)


# ---- 2. the lazy replay ------------------------------------------------------------------
N_LAZY = 20


def _lazy_inputs(rom, n, kind):
    soc0, tc0 = batch_inputs(n, seed=227)
    if kind == "T":   # every cell crosses the 25 degC set-point of the (15, 25, 35) grid
        ramp = np.linspace(22.0, 28.0, N_LAZY).reshape(N_LAZY, 1) * np.ones((1, n))
        return soc0, np.full(n, 22.0), ramp
    sp = np.asarray(rom.SOC_pct, dtype=float)
    for i, k in enumerate((2, 3, 4, 5)):   # a few cells just below a SOC set-point
        soc0[7 * i + 1] = sp[k] - 0.15
    return soc0, tc0, None


def _bracket_changes(x, pts):
    """First step at which each cell's pair of bracketing set-points differs from step 0's
    (0: never): x [steps, n], pts ascending."""
    b = np.searchsorted(pts, x, side="right")
    moved = b != b[0]
    return np.where(moved.any(axis=0), moved.argmax(axis=0), 0)


@pytest.mark.parametrize("env", [{}, {"MPCEKF_FLUSH_PERIOD": "4"}, {"MPCEKF_FLUSH_ROLL": "1"}],
                         ids=["default", "flush4", "roll"])
@pytest.mark.parametrize("kind", ["T", "SOC"])
def test_lazy_replay_is_exact(P, M, monkeypatch, kind, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rom = P.make_synth_rom(lookup="quintic")
    n = 65
    soc0, tc0, ramp = _lazy_inputs(rom, n, kind)
    one = _single(M, rom, n, soc0, tc0, N_LAZY, tc=ramp)
    # the precondition: corners go stale inside the call (a bracket first touched at step >= 3)
    if kind == "T":
        first = _bracket_changes(ramp, np.asarray(rom.T_degC, dtype=float))
        assert np.all(first >= 5), first
    else:
        first = _bracket_changes(one["obs"]["cellSOC"], np.sort(np.asarray(rom.SOC_pct, dtype=float)) / 100)
        assert np.any(first >= 3), first
    many = _split(M, rom, n, soc0, tc0, N_LAZY, tc=ramp)
    _same_run(one, many, f"one call vs {N_LAZY} calls ({kind}, {env})")


# ---- 3. every plant location -------------------------------------------------------------
@pytest.mark.parametrize("where", ["quad_plant", "cell_plant", "k_plant4", "MB", "wide"])
def test_every_plant_location(P, M, monkeypatch, where):
    cfg = None
    if where in ("cell_plant", "k_plant4"):
        monkeypatch.setenv("MPCEKF_QUAD", "0")
    if where == "k_plant4":
        monkeypatch.setenv("MPCEKF_CELL_PLANT", "0")
    if where == "MB":
        cfg = M.make_config(method="MB")
    if where == "wide":
        cfg = M.make_config(Np=20, Nc=10)
    rom = P.make_synth_rom(lookup="quintic")
    n = 65
    soc0, tc0, ramp = _lazy_inputs(rom, n, "T")
    one = _single(M, rom, n, soc0, tc0, N_LAZY, cfg=cfg, tc=ramp)
    many = _split(M, rom, n, soc0, tc0, N_LAZY, cfg=cfg, tc=ramp, ref=True)
    _same_run(one, many, where)


# ---- 4. equals the stage route -----------------------------------------------------------
def test_equals_the_stage_route(P, M):
    rom = P.make_synth_rom()
    n, steps = 96, 20
    soc0, tc = batch_inputs(n, seed=83)
    fused = M.runMPC(rom, soc0, tc, steps, obs=True)
    assert tuple(fused["obs"]) == obs_ref.OBS_FIELDS
    with M.Context(rom, n) as dev:
        dev.init_cells(soc0, tc)
        ud = np.zeros(n)
        for k in range(steps):
            vd, o = dev.OB_step(ud, obs=True)
            zd, _, _ = dev.iterEKF(vd, ud, xind=False)
            assert dev.EKFmatsHandler(None, None, keep=True) is None
            ud, _ = dev.iterMPC(None, zd[:, -1])
            _bits_equal(ud, fused["u"][k], f"u step {k}")
            for f in obs_ref.OBS_FIELDS:
                _bits_equal(fused["obs"][f][k], o[f], f"{f} step {k}")
            _bits_equal(fused["obs"]["Vcell"][k], fused["v"][k], f"obs.Vcell vs v step {k}")


# ---- 5. selection ------------------------------------------------------------------------
def test_selection_keeps_bits_and_order(P, M):
    rom = P.make_synth_rom(lookup="quintic")
    n, steps = 65, 6
    soc0, tc = batch_inputs(n, seed=229)
    full = _single(M, rom, n, soc0, tc, steps)
    for sel in (("negPhise0",), ("Thetae", "negPhise0"), ("posPhis",), "Vcell", ("posPhise", "negSOC")):
        part = _single(M, rom, n, soc0, tc, steps, obs=sel)
        names = (sel,) if isinstance(sel, str) else sel
        assert tuple(part["obs"]) == names                      # the request's order
        for f in names:
            _bits_equal(part["obs"][f], full["obs"][f], f"{sel}: {f}")
        for k in KEYS:
            _bits_equal(part[k], full[k], f"{sel}: {k}")
    # a duplicated slot through the C call: positions follow the request
    lay = rom.obs_layout()
    slots = np.array([lay["Vcell"].start, lay["negPhise0"].start, lay["Vcell"].start, lay["Thetae"].start],
                     dtype=np.int32)
    rec = np.empty((steps, slots.size, n))
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        rc = ctx.L.mpcekf_step_ex_obs(ctx.h, steps, None, None, slots.ctypes.data_as(C.POINTER(C.c_int32)),
                                      slots.size, rec.ctypes.data_as(C.c_void_p), 0)
        assert rc == 0
    _bits_equal(rec[:, 0], full["obs"]["Vcell"], "dup 0")
    _bits_equal(rec[:, 1], full["obs"]["negPhise0"], "dup 1")
    _bits_equal(rec[:, 2], full["obs"]["Vcell"], "dup 2")
    _bits_equal(rec[:, 3], full["obs"]["Thetae"][:, :, 0], "dup 3")


def test_unknown_field_raises_before_any_call(P, M):
    rom = P.make_synth_rom()
    with M.Context(rom, 3) as ctx:      # not initialised: a library call would be MpcekfError
        with pytest.raises(KeyError, match="negPhise9"):
            ctx.step(1, obs=("negPhise0", "negPhise9"))


# ---- 6. nothing else moves ---------------------------------------------------------------
def test_nothing_else_moves(P, M):
    rom = P.make_synth_rom(lookup="quintic")
    n, steps = 257, 8
    soc0, tc = batch_inputs(n, seed=233)
    runs = []
    for obs in (None, ("negPhise0",), True):
        with M.Context(rom, n) as ctx:
            ctx.init_cells(soc0, tc)
            o = ctx.step(steps, outputs=KEYS + ("nexec", "zk"), obs=obs)
            assert ("obs" in o) == (obs is not None)
            runs.append((o, ctx.get_state()))
    (o0, s0) = runs[0]
    for o, s in runs[1:]:
        for k in KEYS + ("zk",):
            _bits_equal(o[k], o0[k], k)
        assert np.array_equal(o["nexec"], o0["nexec"])
        for k in ("bigX", "ekf", "scal", "lam"):
            _bits_equal(s[k], s0[k], f"state {k}")
        assert np.array_equal(s["warn"], s0["warn"]) and np.array_equal(s["status"], s0["status"])


def test_timing_launch_counts(P, M):
    """obs=None launches what mpcekf_step_ex launches; with obs the k_obs_traj launch is inside
    the plant interval, reported every step wherever the plant itself runs."""
    rom = P.make_synth_rom()
    n, steps = 257, 6
    soc0, tc = batch_inputs(n, seed=239)
    counts = {}
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.set_timing(True)
        ctx.get_timing()
        tr = M._lib.Traj()
        assert ctx.L.mpcekf_step_ex(ctx.h, steps, None, C.byref(tr), 0) == 0
        counts["step_ex"] = {k: v[1] for k, v in ctx.get_timing().items()}
        ctx.step(steps, obs=None)
        counts["obs=None"] = {k: v[1] for k, v in ctx.get_timing().items()}
        assert ctx.L.mpcekf_step_ex_obs(ctx.h, steps, None, C.byref(tr), None, 0, None, 0) == 0
        counts["nslots=0"] = {k: v[1] for k, v in ctx.get_timing().items()}
        ctx.step(steps, obs=("negPhise0",))
        counts["obs"] = {k: v[1] for k, v in ctx.get_timing().items()}
    assert counts["obs=None"] == counts["step_ex"] == counts["nslots=0"], counts
    assert counts["obs"]["plant"] == steps, counts
    assert {k: v for k, v in counts["obs"].items() if k != "plant"} == \
           {k: v for k, v in counts["step_ex"].items() if k != "plant"}, counts


# ---- 7. error cells ----------------------------------------------------------------------
def test_error_cells_are_nan_and_neighbours_unaffected(P, M):
    rom = P.make_synth_rom()
    n, steps, bad = 65, 6, [0, 2, 64]

    def run(status):
        with M.Context(rom, n) as ctx:
            ctx.init_cells(*batch_inputs(n, seed=241))
            st = ctx.get_state()
            st["status"] = status
            ctx.set_state(st)
            return ctx.step(steps, obs=True)

    status = np.zeros(n, dtype=np.int32)
    clean = run(status)
    status[bad] = ST_ERROR
    err = run(status)
    keep = np.setdiff1d(np.arange(n), bad)
    for f in obs_ref.OBS_FIELDS:
        assert np.all(np.isnan(err["obs"][f][:, bad])), f
        assert np.all(np.isfinite(clean["obs"][f])), f
        _bits_equal(err["obs"][f][:, keep], clean["obs"][f][:, keep], f)
    for k in KEYS:
        _bits_equal(err[k][:, keep], clean[k][:, keep], k)


# ---- 8. graph replay and device outputs --------------------------------------------------
def test_graph_replay_and_device_outputs(P, M):
    rom = P.make_synth_rom(lookup="quintic")
    n, steps = 65, 5
    soc0, tc = batch_inputs(n, seed=251)
    calls = (("negPhise0", "Thetae"), ("negPhise0", "Thetae"), ("Vcell", "negSOC", "Phie"))
    with M.Context(rom, n) as plain, M.Context(rom, n) as graph:
        plain.init_cells(soc0, tc)
        graph.init_cells(soc0, tc)
        graph.set_graph(True)
        for i, sel in enumerate(calls):
            a, b = plain.step(steps, obs=sel), graph.step(steps, obs=sel)
            _same_run(a, b, f"graph call {i}")
    lay = rom.obs_layout()
    slots = [lay["negPhise0"].start, lay["Vcell"].start, lay["Thetae"].start + 1]
    host = _single(M, rom, n, soc0, tc, steps, obs=("negPhise0", "Vcell", "Thetae"))
    with M.Context(rom, n) as ctx, M.DeviceBuffer((steps, len(slots), n)) as ob, M.DeviceBuffer((steps, n)) as ub:
        ctx.init_cells(soc0, tc)
        ctx.step_device(steps, u=ub, obs=ob, obs_slots=slots)
        rec, u = ob.to_host(), ub.to_host()
    _bits_equal(u, host["u"], "device u")
    _bits_equal(rec[:, 0], host["obs"]["negPhise0"], "device negPhise0")
    _bits_equal(rec[:, 1], host["obs"]["Vcell"], "device Vcell")
    _bits_equal(rec[:, 2], host["obs"]["Thetae"][:, :, 1], "device Thetae(2)")


# ---- 9. arguments ------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_context_still_steps(P, M):
    rom = P.make_synth_rom()
    n = 3
    nobs = rom.obs_layout()["Vcell"].stop
    ip = C.POINTER(C.c_int32)
    rec = np.empty((1, 2, n))
    with M.Context(rom, n) as ctx, M.Context(rom, n) as ref:
        for c in (ctx, ref):
            c.init_cells(*batch_inputs(n, seed=257))
        call = lambda sl, k, out: ctx.L.mpcekf_step_ex_obs(ctx.h, 1, None, None, sl, k, out, 0)
        good = np.array([0, 1], dtype=np.int32)
        for bad in ([0, nobs], [-1, 0]):
            sl = np.array(bad, dtype=np.int32)
            assert call(sl.ctypes.data_as(ip), 2, rec.ctypes.data_as(C.c_void_p)) == E_ARG
            assert b"slot" in ctx.L.mpcekf_last_error()
        assert call(good.ctypes.data_as(ip), -1, rec.ctypes.data_as(C.c_void_p)) == E_ARG
        assert call(good.ctypes.data_as(ip), 2, None) == E_ARG
        assert call(None, 2, rec.ctypes.data_as(C.c_void_p)) == E_ARG
        _same_run(ctx.step(4, obs=True), ref.step(4, obs=True), "after refused calls")


# ---- 10. the gateway ---------------------------------------------------------------------
def test_stepobs_through_gateway(P, M):
    mexshim.build()
    rom = P.make_synth_rom()
    n, steps = 3, 4
    soc0, tc = batch_inputs(n, seed=263)
    lay = rom.obs_layout()
    fields = ("negPhise0", "Thetae", "Vcell")
    idx = np.concatenate([np.arange(lay[f].start, lay[f].stop) for f in fields]).astype(float) + 1.0
    h = mexshim.mex("create", mexshim.rom_struct(rom), {}, 0.0, float(n))
    try:
        mexshim.mex("init", h, soc0, tc, nargout=0)
        u, v, soc, phise, nexec, obs = mexshim.mex("stepobs", h, float(steps), idx[None, :], nargout=6)
        with pytest.raises(mexshim.MexError, match="mpcekf:arg: stepobs: idx.* is not a slot 1..38"):
            mexshim.mex("stepobs", h, 1.0, np.array([[39.0]]), nargout=6)
    finally:
        mexshim.mex("destroy", h, nargout=0)
    ref = _single(M, rom, n, soc0, tc, steps, obs=fields)
    assert obs.shape == (n, idx.size, steps)                     # ncells x numel(idx) x nsteps
    for got, k in ((u, "u"), (v, "v"), (soc, "soc"), (phise, "phise")):
        _bits_equal(got, ref[k].T, f"gateway {k}")
    assert np.array_equal(nexec, ref["nexec"].T)
    _bits_equal(obs[:, 0, :], ref["obs"]["negPhise0"].T, "gateway negPhise0")
    _bits_equal(obs[:, 1:4, :], ref["obs"]["Thetae"].transpose(1, 2, 0), "gateway Thetae")
    _bits_equal(obs[:, 4, :], ref["obs"]["Vcell"].T, "gateway Vcell")
