"""The corner window: between flushes the fused loop keeps each cell's four
active EKF corner records slot-major in a context-owned buffer instead of scattering them back
to their [ncells][NM][20] records every step.  It moves bytes and nothing else, so every
comparison here is BITWISE: window on (MPCEKF_HOT_CORNERS=1, the default) against a window-off
twin (=0) and, where one exists, against the C oracle.  "Outputs" are u, v, soc, phise, nexec
(and zk / boundzk where the call returns them) of every step and get_state()'s ekf, bigX, scal,
lam, warn and status at the end.

MPCEKF_QUAD=0 everywhere (except the quad case): at these batch sizes the default is the
lane-quad k_ekf4, which does not use the window; the lane-per-cell k_cell is what is under test.
"""
import contextlib
import os
from importlib import import_module

import numpy as np
import pytest

from conftest import batch_inputs

pytestmark = pytest.mark.gpu

KEYS = ("u", "v", "soc", "phise", "nexec")
ZKEYS = KEYS + ("zk", "zbk")
STATE = ("ekf", "bigX", "scal", "lam", "warn", "status")
ON = dict(MPCEKF_QUAD=0, MPCEKF_HOT_CORNERS=1)
OFF = dict(MPCEKF_QUAD=0, MPCEKF_HOT_CORNERS=0)
N, STEPS, FLUSH = 200, 300, 64   # 200 cells: three full waves and a partial one


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")   # the bench's tables; set-points 15 / 25 / 35 degC, SOC every 5 %


@contextlib.contextmanager
def _env(**env):
    """The host switches are read at context creation (tests/test_gpu_parity.py _run_with_env)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx(M, rom, n, env, cfg=None):
    with _env(**env):
        return M.Context(rom, n, cfg)


def _bitwise(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def _same_run(a, b, keys, what):
    for k in keys:
        _bitwise(a[k], b[k], f"{what}: {k}")
    for k in STATE:
        _bitwise(a["state"][k], b["state"][k], f"{what}: state {k}")


def _run(M, rom, soc0, tc, chunks, env, cfg=None, tct=None, keys=KEYS, graph=False):
    """The fused loop in calls of chunks[i] steps; the per-step outputs concatenated, the state
    after the last call."""
    with _ctx(M, rom, len(soc0), env, cfg) as ctx:
        ctx.init_cells(soc0, tc)
        if graph:
            ctx.set_graph(True)
        parts, k0 = [], 0
        for k in chunks:
            parts.append(ctx.step(k, outputs=keys, tc=None if tct is None else tct[k0:k0 + k]))
            k0 += k
        out = {k: np.concatenate([p[k] for p in parts]) for k in keys}
        out["state"] = ctx.get_state()
    return out


# ---------------------------------------------------------------------------
# inputs that change corner sets while the window holds them
# ---------------------------------------------------------------------------
def crossing_inputs(rom, n, steps):
    """SOC0 0.02..0.6 % below a SOC set-point (10 .. 35 %), so the estimate crosses it within
    the first steps and the next ones later in the run; a per-step temperature 25 +- 3 degC
    (period 90 steps, a phase per cell) that passes the 25 degC set-point in both directions."""
    rng = np.random.Generator(np.random.PCG64(0xC0 + n))
    soc0 = rng.choice(rom.SOC_pct[2:8], n) - rng.uniform(0.02, 0.6, n)
    k = np.arange(steps)[:, None]
    tct = 25.0 + 3.0 * np.sin(2 * np.pi * (k / 90.0 + rng.uniform(0, 1, n)[None, :]))
    return soc0, tct[0].copy(), np.ascontiguousarray(tct)


def crossing_floor(rom, soc, tct):
    """From a trajectory of the estimate's SOC [steps, n] (fraction) and the temperatures: the
    fraction of cells whose SOC set-point interval changes, of those whose T interval changes,
    and the flush windows (steps 64 w + 1 .. 64 w + 64) in which some cell changes either, not
    counting a change on a window's first step (the window is empty there)."""
    iz = np.searchsorted(rom.SOC_pct / 100.0, soc, side="right")
    it = np.searchsorted(rom.T_degC, tct, side="right")
    dz, dt = iz[1:] != iz[:-1], it[1:] != it[:-1]
    inside = (np.arange(1, soc.shape[0]) % FLUSH != 0)[:, None]   # row k is step k + 1; k % 64 == 0 opens a window
    dz, dt = dz & inside, dt & inside
    wins = sorted(set((np.nonzero((dz | dt).any(axis=1))[0] + 1) // FLUSH))
    return dz.any(axis=0).mean(), dt.any(axis=0).mean(), wins


@pytest.fixture(scope="module")
def crossing(rom, oc, M):
    """The crossing case: its inputs, the oracle's trajectory and the window-off and window-on
    runs (one call, boundzk on), computed once for the tests below."""
    soc0, tc0, tct = crossing_inputs(rom, N, STEPS)
    ref = oc.run(rom, soc0, tc0, STEPS, nthreads=8, tc_traj=tct, traj=True)
    cfg = M.make_config(bounds=True)
    off = _run(M, rom, soc0, tc0, [STEPS], OFF, cfg, tct, ZKEYS)
    on = _run(M, rom, soc0, tc0, [STEPS], ON, cfg, tct, ZKEYS)
    return dict(soc0=soc0, tc0=tc0, tct=tct, ref=ref, cfg=cfg, off=off, on=on)


def test_crossings_match_oracle_and_twin(rom, crossing):
    """1. Corner sets change under the window (the floor is asserted on the oracle's own
    trajectory first), and the run is the oracle's and the window-off twin's bit for bit."""
    ref = crossing["ref"]
    fz, ft, wins = crossing_floor(rom, ref["soc"], crossing["tct"])
    print(f"cells changing SOC interval {fz:.2f}, T interval {ft:.2f}, flush windows with a change {wins}")
    assert fz >= 0.25 and ft >= 0.25, (fz, ft)
    assert len(wins) >= 3, wins
    assert (ref["status"] == 0).all()
    pairs = dict(u="u", v="v", soc="soc", phise="phise", nexec="nexec", zk="zk_traj", zbk="zbk_traj")
    for arm in ("on", "off"):
        for k, rk in pairs.items():
            _bitwise(crossing[arm][k], ref[rk], f"window {arm} vs oracle: {k}")
        _bitwise(crossing[arm]["state"]["status"], ref["status"], f"window {arm} vs oracle: status")
    _same_run(crossing["on"], crossing["off"], ZKEYS, "window on vs off")


@pytest.mark.parametrize("period", [1, 4, 7, 64])
def test_flush_periods(rom, M, crossing, period):
    """2. Any flush period gives the same outputs (at period 1 the window never hits)."""
    c = crossing
    out = _run(M, rom, c["soc0"], c["tc0"], [STEPS], dict(ON, MPCEKF_FLUSH_PERIOD=period), c["cfg"], c["tct"], ZKEYS)
    _same_run(out, c["off"], ZKEYS, f"flush period {period}")


def test_call_splitting_and_state(rom, M, crossing):
    """3. One call of N steps equals calls of [1, 63, 64, 65, 7, ...] steps; get_state between
    the calls equals a window-off twin's; set_state of an earlier checkpoint followed by more
    steps equals the twin's."""
    c = crossing
    chunks = [1, 63, 64, 65, 7, STEPS - 200]
    out = _run(M, rom, c["soc0"], c["tc0"], chunks, ON, c["cfg"], c["tct"], ZKEYS)
    _same_run(out, c["on"], ZKEYS, "split calls vs one call")
    with _ctx(M, rom, N, ON, c["cfg"]) as a, _ctx(M, rom, N, OFF, c["cfg"]) as b:
        snaps, k0 = {}, 0
        for x in (a, b):
            x.init_cells(c["soc0"], c["tc0"])
        for i, k in enumerate(chunks[:5]):
            ra, rb = (x.step(k, outputs=ZKEYS, tc=c["tct"][k0:k0 + k]) for x in (a, b))
            k0 += k
            sa, sb = a.get_state(), b.get_state()
            for key in ZKEYS:
                _bitwise(ra[key], rb[key], f"call {i}: {key}")
            for key in STATE:
                _bitwise(sa[key], sb[key], f"state after call {i}: {key}")
            if i == 1:
                snaps = dict(a=sa, b=sb, k0=k0)
        # back to the checkpoint after 64 steps, then 70 more (over a flush)
        a.set_state(snaps["a"])
        b.set_state(snaps["b"])
        k0 = snaps["k0"]
        ra, rb = (x.step(70, outputs=ZKEYS, tc=c["tct"][k0:k0 + 70]) for x in (a, b))
        sa, sb = a.get_state(), b.get_state()
    for key in ZKEYS:
        _bitwise(ra[key], rb[key], f"after set_state: {key}")
        _bitwise(ra[key], c["on"][key][k0:k0 + 70], f"after set_state vs the uninterrupted run: {key}")
    for key in STATE:
        _bitwise(sa[key], sb[key], f"state after set_state: {key}")


def test_stage_calls_between_fused_calls(rom, M, crossing):
    """4. A plant_step / ekf_step / linearize / mpc_step round between two fused calls."""
    c = crossing
    res = []
    for env in (ON, OFF):
        with _ctx(M, rom, N, env, c["cfg"]) as ctx:
            ctx.init_cells(c["soc0"], c["tc0"])
            r1 = ctx.step(70, outputs=ZKEYS, tc=c["tct"][:70])
            uk = r1["u"][-1].copy()
            v = ctx.OB_step(uk)
            zk, zb, xind = ctx.iterEKF(v, uk)
            lin = ctx.EKFmatsHandler(zk, xind)
            uk2, ne = ctx.iterMPC(lin, zk[:, -1])
            r2 = ctx.step(70, outputs=ZKEYS, tc=c["tct"][71:141])
            res.append(dict(r1=r1, r2=r2, v=v, zk=zk, zb=zb, lin=np.asarray(lin), uk2=uk2, ne=ne,
                            xm=np.asarray(xind["model"]), state=ctx.get_state()))
    a, b = res
    for key in ZKEYS:
        _bitwise(a["r1"][key], b["r1"][key], f"first fused call: {key}")
        _bitwise(a["r2"][key], b["r2"][key], f"second fused call: {key}")
    for key in ("v", "zk", "zb", "lin", "uk2", "ne", "xm"):
        _bitwise(a[key], b[key], f"stage round: {key}")
    for key in STATE:
        _bitwise(a["state"][key], b["state"][key], f"state: {key}")


@pytest.mark.parametrize("lookup", ["linear", "quintic"])
def test_lockout_and_error_cells(P, oc, M, lookup):
    """5a. tests/test_gpu_parity.py test_lockout_and_error_cells' inputs: the early returns
    leave the window as they found it."""
    rom = P.make_synth_rom(lookup=lookup)
    soc0 = np.array([10.0, 130.0, 20.0, 130.0])
    tc = np.array([25.0, 25.0, 15.0, 35.0])
    ref = oc.run(rom, soc0, tc, 30, nthreads=1)
    on, off = (_run(M, rom, soc0, tc, [30], env) for env in (ON, OFF))
    _same_run(on, off, KEYS, "window on vs off")
    assert (on["state"]["status"][[1, 3]] & 1).all()
    _bitwise(on["state"]["status"], ref["status"], "status vs oracle")
    for k in ("u", "v", "soc", "phise"):
        _bitwise(on[k], ref[k], f"vs oracle: {k}")


def test_single_temperature_rom(P, oc, M):
    """5b. A ROM with one temperature set-point: every cell's corners repeat (dup), so no cell
    uses the window; equal to the twin and the oracle."""
    rom = P.make_synth_rom(T_degC=(25.0,), lookup="quintic")
    soc0, tc = batch_inputs(100, seed=31)
    soc0[:6] = rom.SOC_pct[2:8] - 0.05
    ref = oc.run(rom, soc0, tc, 80, nthreads=8)
    on, off = (_run(M, rom, soc0, tc, [80], env) for env in (ON, OFF))
    _same_run(on, off, KEYS, "window on vs off")
    for k in KEYS:
        _bitwise(on[k], ref[k], f"vs oracle: {k}")


def _route_inputs(rom, n, steps):
    soc0, tc0, tct = crossing_inputs(rom, n, steps)
    return soc0, tc0, tct


@pytest.mark.parametrize("route", ["np20", "switch_off", "graph", "split"])
def test_routes(rom, M, route):
    """6a. The other forms of the fused step that run iterEKF in k_cell: window on == off."""
    n, steps = 136, 80
    soc0, tc0, tct = _route_inputs(rom, n, steps)
    cfg = {"np20": dict(Np=20, Nc=10), "switch_off": dict(constraints=(1, 0, 1))}.get(route, {})
    cfg = M.make_config(bounds=True, **cfg)
    extra = dict(MPCEKF_SPLIT_CELL=1) if route == "split" else {}
    chunks = [40, 40] if route == "graph" else [steps]   # the second call replays the captured graph
    on, off = (_run(M, rom, soc0, tc0, chunks, dict(env, **extra), cfg, tct, ZKEYS, graph=route == "graph")
               for env in (ON, OFF))
    _same_run(on, off, ZKEYS, route)


def test_route_step_summary(rom, M):
    """6b. step_summary: the summary record and the state."""
    n, steps = 136, 80
    soc0, tc0, tct = _route_inputs(rom, n, steps)
    res = []
    for env in (ON, OFF):
        with _ctx(M, rom, n, env) as ctx:
            ctx.init_cells(soc0, tc0)
            ctx.summary_begin(reach=0.2)
            ctx.step_summary(steps, tc=tct)
            res.append((ctx.get_summary(), ctx.get_state()))
            ctx.summary_end()
    for k in res[0][0]:
        _bitwise(res[0][0][k], res[1][0][k], f"summary {k}")
    for k in STATE:
        _bitwise(res[0][1][k], res[1][1][k], f"state {k}")


def test_route_thermal(rom, M):
    """6c. A thermal context: the model drives the temperature through the 25 degC set-point."""
    n, steps = 136, 80
    soc0, _, _ = _route_inputs(rom, n, steps)
    rng = np.random.Generator(np.random.PCG64(77))
    T0, Tamb = rng.uniform(24.0, 26.0, n), rng.uniform(15.0, 35.0, n)
    ocv = M.thermal_ocv(rom)
    res = []
    for env in (ON, OFF):
        with _ctx(M, rom, n, env) as ctx:
            ctx.init_cells(soc0, T0)
            ctx.thermal_begin(40.0, 0.5, Tamb, ocv, T0=T0)
            out = ctx.step(steps, thermal=("temp", "heat"))
            res.append((out, ctx.thermal_get(), ctx.get_state()))
    (oa, ta, sa), (ob, tb, sb) = res
    for k in KEYS + ("temp", "heat"):
        _bitwise(oa[k], ob[k], k)
    for k in ta:
        _bitwise(ta[k], tb[k], f"thermal {k}")
    for k in STATE:
        _bitwise(sa[k], sb[k], f"state {k}")


def test_route_step_ex_obs(rom, M):
    """6d. step_ex_obs with one slot."""
    n, steps = 136, 80
    soc0, tc0, tct = _route_inputs(rom, n, steps)
    res = []
    for env in (ON, OFF):
        with _ctx(M, rom, n, env) as ctx:
            ctx.init_cells(soc0, tc0)
            out = ctx.step(steps, tc=tct, obs="cellSOC")
            res.append((out, ctx.get_state()))
    for k in KEYS:
        _bitwise(res[0][0][k], res[1][0][k], k)
    _bitwise(res[0][0]["obs"]["cellSOC"], res[1][0]["obs"]["cellSOC"], "obs cellSOC")
    for k in STATE:
        _bitwise(res[0][1][k], res[1][1][k], f"state {k}")


@pytest.mark.parametrize("kind", ["mb", "quad", "roll"])
def test_ineligible_contexts(rom, M, kind):
    """7. Contexts that get no window run with MPCEKF_HOT_CORNERS=1 and equal their twins."""
    n, steps = 136, 80
    soc0, tc0, tct = _route_inputs(rom, n, steps)
    cfg = M.make_config(bounds=True, **(dict(method="MB") if kind == "mb" else {}))
    extra = dict(mb={}, quad=dict(MPCEKF_QUAD=1), roll=dict(MPCEKF_FLUSH_ROLL=1))[kind]
    on, off = (_run(M, rom, soc0, tc0, [steps], dict(env, **extra), cfg, tct, ZKEYS) for env in (ON, OFF))
    _same_run(on, off, ZKEYS, kind)
