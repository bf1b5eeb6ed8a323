"""GPU: the per-cell charge summary along the fused loop (mpcekf_summary_begin / _step_summary /
_get_summary / _summary_end; k_summary over the SUM_WIN-row window).

The expected record always comes from a twin context that runs the same inputs through the
existing Context.step(...) and whose trajectories tests/summary_ref.py reduces; never from the
code under test.  Every field is compared with np.array_equal on the uint64 views.

Shapes: 130 cells (two full waves and a 2-lane tail, inside a partial 256-thread block) and 150
steps (two full 64-step windows and one of 22); Np = 20 / Nc = 10: 66 cells x 70 steps.
"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import mexshim
import summary_ref as sr
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

N, STEPS = 130, 150
KEYS = ("u", "v", "soc", "phise", "nexec")
ST_ERROR = 1
E_ARG, E_STATE = -1, -5
NO_OBS = tuple(k for k in sr.FIELDS if not k.startswith("obs_"))


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def _limits(n):
    """Per-cell limits that vary across the batch (a protocol sweep)."""
    return dict(v_max=np.linspace(3.9, 4.1, n), Crate=np.linspace(1.5, 3.0, n))


ROUTES = {
    "ob": dict(cfg={}, n=N, steps=STEPS),
    "mb": dict(cfg=dict(method="MB"), n=N, steps=STEPS),
    "switch": dict(cfg=dict(constraints=(1, 1, 0)), n=N, steps=STEPS),
    "percell": dict(cfg={}, n=N, steps=STEPS, limits=True),
    "wide": dict(cfg=dict(Np=20, Nc=10), n=66, steps=70),
}


def _twin(M, rom, n, steps, cfg=None, limits=None, tc=None, obs=None, status=None):
    """The existing per-step route: Context.step's trajectories and the final state."""
    soc0, tc0 = batch_inputs(n)
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc0)
        if status is not None:
            st = ctx.get_state()
            st["status"] = status
            ctx.set_state(st)
        if limits:
            ctx.set_limits(**limits)
        out = ctx.step(steps, outputs=KEYS, tc=tc, obs=obs)
        out["state"] = ctx.get_state()
    return out


def _reach(twin):
    """The twin's soc at step 60 (a counted step: the cell then reaches it at step 60 at the
    latest, earlier where the estimate was already there), +inf for every fifth cell."""
    r = twin["soc"][59].copy()
    r[::5] = np.inf
    return r


def _floor(ref, steps):
    """On the twin alone: the threshold path is not silently empty."""
    t = ref["t_reach"]
    assert ((t > 0) & (t < steps)).mean() >= 0.25, t
    assert (t == 0).any()


def _summary(M, rom, n, calls, cfg=None, limits=None, tc=None, reach=None, obs=None, status=None, graph=False):
    soc0, tc0 = batch_inputs(n)
    with M.Context(rom, n, cfg) as ctx:
        ctx.init_cells(soc0, tc0)
        if status is not None:
            st = ctx.get_state()
            st["status"] = status
            ctx.set_state(st)
        if limits:
            ctx.set_limits(**limits)
        ctx.set_graph(graph)
        ctx.summary_begin(reach=reach, obs=obs)
        k = 0
        for m in calls:
            ctx.step_summary(m, tc=None if tc is None else tc[k:k + m])
            k += m
        return ctx.get_summary(), ctx.get_state()


def _state_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if a[k].dtype.kind == "f":
            sr.bits_equal(a[k], b[k], f"{what}: state {k}")
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: state {k}"


# ---- 1. parity per route ---------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_parity_per_route(M, rom, route):
    r = ROUTES[route]
    n, steps = r["n"], r["steps"]
    cfg = M.make_config(**r["cfg"])
    lim = _limits(n) if r.get("limits") else None
    twin = _twin(M, rom, n, steps, cfg, lim)
    reach = _reach(twin)
    ref = sr.reduce(twin, reach=reach, max_hild=cfg.max_hild)
    _floor(ref, steps)
    assert (ref["steps"] == steps).mean() >= 0.75 and (ref["nexec_sum"] > 0).any()
    got, st = _summary(M, rom, n, (steps,), cfg, lim, reach=reach)
    assert tuple(got) == sr.FIELDS
    sr.same_record(got, ref, route)
    _state_equal(st, twin["state"], route)


# ---- 2. the plant's slot ---------------------------------------------------------------------
def test_plant_slot(M, rom):
    twin = _twin(M, rom, N, STEPS, obs="negPhise0")
    reach = _reach(twin)
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    assert np.isfinite(ref["obs_min"]).all() and (ref["obs_min_step"] >= 1).all()
    assert (ref["obs_min"] != ref["phise_min"]).any()      # the plant's margin is not the EKF's estimate
    got, _ = _summary(M, rom, N, (STEPS,), reach=reach, obs="negPhise0")
    sr.same_record(got, ref, "negPhise0")
    # a vector field's entry, by (field, index)
    twin = _twin(M, rom, N, 70, obs="Thetae")
    ref = sr.reduce(twin, obs=twin["obs"]["Thetae"][:, :, 1])
    got, _ = _summary(M, rom, N, (70,), obs=("Thetae", 1))
    sr.same_record(got, ref, "Thetae(2)")


# ---- 3. accumulation across calls --------------------------------------------------------------
def test_accumulation_across_calls(M, rom):
    twin = _twin(M, rom, N, STEPS, obs="negPhise0")
    reach = _reach(twin)
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    got, st = _summary(M, rom, N, (70, 1, 79), reach=reach, obs="negPhise0")
    sr.same_record(got, ref, "70 + 1 + 79")
    _state_equal(st, twin["state"], "70 + 1 + 79")


def test_set_limits_between_calls(M, rom):
    soc0, tc0 = batch_inputs(N)
    lim = _limits(N)
    with M.Context(rom, N) as tw:
        tw.init_cells(soc0, tc0)
        a = tw.step(70, outputs=KEYS)
        tw.set_limits(**lim)
        b = tw.step(80, outputs=KEYS)
    traj = {k: np.concatenate([a[k], b[k]]) for k in KEYS}
    reach = _reach(traj)
    ref = sr.reduce(traj, reach=reach)
    whole = sr.reduce(_twin(M, rom, N, STEPS), reach=reach)
    assert any(not np.array_equal(ref[k], whole[k], equal_nan=True) for k in ("u_min", "v_max", "u_sum"))
    with M.Context(rom, N) as ctx:
        ctx.init_cells(soc0, tc0)
        ctx.summary_begin(reach=reach)
        ctx.step_summary(70)
        ctx.set_limits(**lim)
        ctx.step_summary(1)
        ctx.step_summary(79)
        got = ctx.get_summary()
    sr.same_record(got, ref, "set_limits after 70 steps")


# ---- 4. per-step temperatures ------------------------------------------------------------------
@pytest.mark.parametrize("method", ["OB", "MB"])
def test_per_step_temperatures(M, rom, method):
    """A temperature ramp [150, n] through the window-by-window upload (a 100-step call) and the
    one-piece upload (a 50-step call), with the plant inside k_ekf4 (OB) and as k_plant (MB)."""
    cfg = M.make_config(method=method)
    _, tc0 = batch_inputs(N)
    tc = tc0[None, :] + np.linspace(0.0, 4.0, STEPS)[:, None]
    twin = _twin(M, rom, N, STEPS, cfg, tc=tc, obs="negPhise0")
    plain = _twin(M, rom, N, STEPS, cfg)
    assert not np.array_equal(twin["v"], plain["v"], equal_nan=True)
    reach = _reach(twin)
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    got, st = _summary(M, rom, N, (100, 50), cfg, tc=tc, reach=reach, obs="negPhise0")
    sr.same_record(got, ref, f"tc {method}")
    _state_equal(st, twin["state"], f"tc {method}")


# ---- 5. a cell in error ------------------------------------------------------------------------
def test_error_cell(M, rom):
    bad = 64
    status = np.zeros(N, dtype=np.int32)
    clean = _twin(M, rom, N, STEPS, obs="negPhise0")
    reach = _reach(clean)
    status[bad] = ST_ERROR
    twin = _twin(M, rom, N, STEPS, obs="negPhise0", status=status)
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    got, _ = _summary(M, rom, N, (STEPS,), reach=reach, obs="negPhise0", status=status)
    sr.same_record(got, ref, "error cell")
    assert got["steps"][bad] == 0 and got["err_step"][bad] == 1 and got["seen"][bad] == STEPS
    for k in ("u_min", "u_max", "v_max", "v_min", "phise_min", "nexec_max", "obs_min", "obs_max", "u_last"):
        assert np.isnan(got[k][bad]), k
    for k in ("u_min_step", "v_max_step", "phise_min_step", "obs_min_step", "obs_max_step", "t_reach", "u_sum", "nsat"):
        assert got[k][bad] == 0, k
    keep = np.arange(N) != bad
    ref_clean = sr.reduce(clean, reach=reach, obs=clean["obs"]["negPhise0"])
    for k in sr.FIELDS:
        sr.bits_equal(got[k][keep], ref_clean[k][keep], f"neighbours: {k}")


# ---- 6. nothing else moves ---------------------------------------------------------------------
def test_nothing_else_moves(M, rom):
    soc0, tc0 = batch_inputs(N)
    with M.Context(rom, N) as ctx, M.Context(rom, N) as never:
        ctx.init_cells(soc0, tc0)
        never.init_cells(soc0, tc0)
        ctx.summary_begin(reach=0.3, obs="negPhise0")
        ctx.step_summary(STEPS)
        never.step(STEPS, outputs=())
        _state_equal(ctx.get_state(), never.get_state(), "step_summary vs step")
        first = ctx.get_summary()
        assert (first["seen"] == STEPS).all()
        ctx.summary_begin()                               # a second begin: an all-reset record
        sr.same_record(ctx.get_summary(), sr.reset(N), "second begin")
        ctx.summary_end()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: get_summary"):
            ctx.get_summary()
        a, b = ctx.step(40, outputs=KEYS), never.step(40, outputs=KEYS)
        for k in KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        _state_equal(ctx.get_state(), never.get_state(), "after summary_end")
        ctx.summary_end()                                 # a no-op without a begin


# ---- 7. graph replay ---------------------------------------------------------------------------
def test_graph_replay(M, rom):
    """Three same-shape calls of 4 steps replay one captured graph: the step index comes from
    the record, so steps 5..12 are numbered 5..12 (a call-relative index would give 1..4)."""
    twin = _twin(M, rom, N, 12, obs="negPhise0")
    reach = twin["soc"][6].copy()                         # reached at step 7 at the latest: inside the second call
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    assert (ref["t_reach"] > 4).any() and (ref["v_max_step"] > 4).any()
    plain, st0 = _summary(M, rom, N, (4, 4, 4), reach=reach, obs="negPhise0")
    graph, st1 = _summary(M, rom, N, (4, 4, 4), reach=reach, obs="negPhise0", graph=True)
    sr.same_record(plain, ref, "ungraphed")
    sr.same_record(graph, ref, "graph replay")
    _state_equal(st1, st0, "graph replay")


# ---- 8. refusals -------------------------------------------------------------------------------
def test_refusals_leave_the_context_stepping(M, rom):
    n = 3
    soc0, tc0 = batch_inputs(n)
    nobs = rom.obs_layout()["Vcell"].stop
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    vals = np.zeros((2, n))
    with M.Context(rom, n) as ctx, M.Context(rom, n) as ref:
        L, h = ctx.L, ctx.h
        for c in (ctx, ref):
            c.init_cells(soc0, tc0)
        ids = np.array([0, 1], dtype=np.int32)
        assert L.mpcekf_get_summary(h, 2, ids.ctypes.data_as(ip), vals.ctypes.data_as(dp)) == E_STATE
        assert L.mpcekf_step_summary(h, 1, None) == E_STATE
        for slot in (nobs, -2):
            assert L.mpcekf_summary_begin(h, None, slot) == E_ARG
            assert b"obs_slot" in L.mpcekf_last_error()
        assert L.mpcekf_step_summary(h, 1, None) == E_STATE          # a refused begin began nothing
        ctx.summary_begin(obs="negPhise0")
        assert L.mpcekf_step_summary(h, -1, None) == E_ARG
        twice = np.array([4, 4], dtype=np.int32)
        assert L.mpcekf_get_summary(h, 2, twice.ctypes.data_as(ip), vals.ctypes.data_as(dp)) == E_ARG
        assert b"twice" in L.mpcekf_last_error()
        unknown = np.array([0, len(sr.FIELDS)], dtype=np.int32)
        assert L.mpcekf_get_summary(h, 2, unknown.ctypes.data_as(ip), vals.ctypes.data_as(dp)) == E_ARG
        assert L.mpcekf_get_summary(h, 0, ids.ctypes.data_as(ip), vals.ctypes.data_as(dp)) == E_ARG
        assert L.mpcekf_get_summary(h, 2, None, vals.ctypes.data_as(dp)) == E_ARG
        assert L.mpcekf_get_summary(h, 2, ids.ctypes.data_as(ip), None) == E_ARG
        sr.same_record(ctx.get_summary(), sr.reset(n), "refused calls accumulate nothing")
        ctx.step_summary(5)
        tw = ref.step(5, outputs=KEYS, obs="negPhise0")
        sr.same_record(ctx.get_summary(), sr.reduce(tw, obs=tw["obs"]["negPhise0"]), "after refused calls")
        a, b = ctx.step(4, outputs=KEYS), ref.step(4, outputs=KEYS)
        for k in KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 9. the gateway ----------------------------------------------------------------------------
def test_summary_through_gateway(M, rom):
    mexshim.build()
    n, steps = 5, 70
    soc0, tc0 = batch_inputs(n)
    twin = _twin(M, rom, n, steps, obs="negPhise0")
    reach = twin["soc"][59].copy()
    reach[0] = np.inf
    ref = sr.reduce(twin, reach=reach, obs=twin["obs"]["negPhise0"])
    slot = float(rom.obs_layout()["negPhise0"].start + 1)          # 1-based
    h = mexshim.mex("create", mexshim.rom_struct(rom), {}, 0.0, float(n))
    try:
        mexshim.mex("init", h, soc0, tc0, nargout=0)
        with pytest.raises(mexshim.MexError, match="mpcekf:lib: mpcekf error -5"):
            mexshim.mex("getsummary", h)
        with pytest.raises(mexshim.MexError, match="mpcekf:arg: summarybegin: slot = 39 is not a slot 1..38"):
            mexshim.mex("summarybegin", h, reach, 39.0, nargout=0)
        with pytest.raises(mexshim.MexError, match=r"mpcekf:arg: summarybegin: reach \(ncells\)"):
            mexshim.mex("summarybegin", h, reach[:4].copy(), slot, nargout=0)
        mexshim.mex("summarybegin", h, reach, slot, nargout=0)
        mexshim.mex("stepsummary", h, 30.0, nargout=0)
        mexshim.mex("stepsummary", h, float(steps - 30), np.zeros((0, 0)), nargout=0)
        s = mexshim.mex("getsummary", h)
        mexshim.mex("summaryend", h, nargout=0)
        with pytest.raises(mexshim.MexError, match="mpcekf:lib: mpcekf error -5"):
            mexshim.mex("getsummary", h)
    finally:
        mexshim.mex("destroy", h, nargout=0)
    assert tuple(s) == sr.FIELDS
    for k in sr.FIELDS:
        assert s[k].shape == (n, 1), k                               # column vectors
        sr.bits_equal(s[k][:, 0], ref[k], f"gateway {k}")
