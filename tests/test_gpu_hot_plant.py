"""The plant window: between flushes the fused loop keeps each cell's four plant
corner states slot-major in a context-owned buffer (KState::hotp_*) instead of gathering them
from, and scattering them back to, bigx / ts_plant every step.  It moves bytes and nothing else,
so every comparison here is BITWISE: window on (MPCEKF_HOT_PLANT=1, the default) against a twin
with MPCEKF_HOT_PLANT=0 and, where the C oracle covers the route, against the oracle.  "Outputs"
are u, v, soc, phise, nexec (and zk / boundzk where the call returns them) of every step and
get_state()'s ekf, bigX, scal, lam, warn and status at the end; bigX is the field a lost or stale
write-back of the window would corrupt.

MPCEKF_QUAD=0 everywhere (except the quad case): at these batch sizes the default is the
lane-quad k_ekf4, which has no window; k_cell's cell_plant is what is under test.
"""
import numpy as np
import pytest

from conftest import batch_inputs
from test_gpu_hot_corners import (KEYS, STATE, ZKEYS, _bitwise, _ctx, _run, _same_run, crossing_floor,
                                  crossing_inputs)

pytestmark = pytest.mark.gpu

ON = dict(MPCEKF_QUAD=0, MPCEKF_HOT_PLANT=1)
OFF = dict(MPCEKF_QUAD=0, MPCEKF_HOT_PLANT=0)
N, STEPS, FLUSH = 200, 300, 64   # 200 cells: three full waves and a partial one; four flushes and the final one


@pytest.fixture(scope="module")
def M(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")   # the bench's tables; set-points 15 / 25 / 35 degC, SOC every 5 %


def _run_obs(M, rom, soc0, tc0, tct, env, obs, steps, cfg=None):
    """One step_ex_obs call: the per-step outputs, the obs dict and the state."""
    with _ctx(M, rom, len(soc0), env, cfg) as ctx:
        ctx.init_cells(soc0, tc0)
        out = ctx.step(steps, tc=tct[:steps], obs=obs)
        out["state"] = ctx.get_state()
    return out


@pytest.fixture(scope="module")
def crossing(rom, oc, M):
    """The crossing case: its inputs, the oracle's trajectory, the window-off and window-on runs
    (one call, boundzk on) and the window-off twin's plant cellSOC, computed once."""
    soc0, tc0, tct = crossing_inputs(rom, N, STEPS)
    ref = oc.run(rom, soc0, tc0, STEPS, nthreads=8, tc_traj=tct, traj=True)
    cfg = M.make_config(bounds=True)
    off = _run(M, rom, soc0, tc0, [STEPS], OFF, cfg, tct, ZKEYS)
    on = _run(M, rom, soc0, tc0, [STEPS], ON, cfg, tct, ZKEYS)
    obs_off = _run_obs(M, rom, soc0, tc0, tct, OFF, "cellSOC", STEPS, cfg)
    return dict(soc0=soc0, tc0=tc0, tct=tct, ref=ref, cfg=cfg, off=off, on=on, obs_off=obs_off)


def test_crossings_match_oracle_and_twin(rom, crossing):
    """1. The plant's corner sets change while the window holds them.  The floors are asserted on
    the plant's own SOC (obs.cellSOC of the window-off twin, whose code path does not know the
    window: the oracle's binding returns the estimate's SOC only) and the given temperatures;
    then the run is the oracle's and the twin's bit for bit."""
    c = crossing
    soc_plant = c["obs_off"]["obs"]["cellSOC"]
    # crossing_floor leaves out a change on a flush window's first step (the window is empty
    # there), so every figure below counts changes that meet a filled window
    fz, ft, wins = crossing_floor(rom, soc_plant, c["tct"])
    print(f"plant: cells changing SOC interval {fz:.2f}, T interval {ft:.2f}, flush windows with a change {wins}")
    assert fz >= 0.5 and ft >= 0.25, (fz, ft)
    assert len(wins) >= 3, wins
    ref = c["ref"]
    assert (ref["status"] == 0).all()
    pairs = dict(u="u", v="v", soc="soc", phise="phise", nexec="nexec", zk="zk_traj", zbk="zbk_traj")
    for arm in ("on", "off"):
        for k, rk in pairs.items():
            _bitwise(c[arm][k], ref[rk], f"window {arm} vs oracle: {k}")
        _bitwise(c[arm]["state"]["status"], ref["status"], f"window {arm} vs oracle: status")
    _same_run(c["on"], c["off"], ZKEYS, "window on vs off")


def test_call_splitting(rom, M, crossing):
    """2a. Calls of [1, 63, 64, 100, 72] steps against one call of 300."""
    c = crossing
    out = _run(M, rom, c["soc0"], c["tc0"], [1, 63, 64, 100, 72], ON, c["cfg"], c["tct"], ZKEYS)
    _same_run(out, c["off"], ZKEYS, "split calls vs the twin's one call")


def test_flush_period_4(rom, M, crossing):
    """2b. MPCEKF_FLUSH_PERIOD=4."""
    c = crossing
    out = _run(M, rom, c["soc0"], c["tc0"], [STEPS], dict(ON, MPCEKF_FLUSH_PERIOD=4), c["cfg"], c["tct"], ZKEYS)
    _same_run(out, c["off"], ZKEYS, "flush period 4")


@pytest.mark.parametrize("corners,plant", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_window_combinations(rom, M, crossing, corners, plant):
    """3. The corner window and the plant window switch independently."""
    c = crossing
    env = dict(MPCEKF_QUAD=0, MPCEKF_HOT_CORNERS=corners, MPCEKF_HOT_PLANT=plant)
    out = _run(M, rom, c["soc0"], c["tc0"], [130], env, c["cfg"], c["tct"], ZKEYS)
    ref = c["ref"]
    for k, rk in dict(u="u", v="v", soc="soc", phise="phise", nexec="nexec", zk="zk_traj", zbk="zbk_traj").items():
        _bitwise(out[k], ref[rk][:130], f"corners {corners} plant {plant} vs oracle: {k}")
    if (corners, plant) != (1, 0):
        twin = _run(M, rom, c["soc0"], c["tc0"], [130], dict(env, MPCEKF_HOT_CORNERS=1, MPCEKF_HOT_PLANT=0), c["cfg"],
                    c["tct"], ZKEYS)
        _same_run(out, twin, ZKEYS, f"corners {corners} plant {plant} vs the default twin")


@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_partial_waves(rom, oc, M, n):
    """4. Batch sizes round a wave, 130 steps (two flushes and the final one)."""
    steps = 130
    soc0, tc0, tct = crossing_inputs(rom, n, steps)
    ref = oc.run(rom, soc0, tc0, steps, nthreads=8, tc_traj=tct)
    on, off = (_run(M, rom, soc0, tc0, [steps], env, None, tct) for env in (ON, OFF))
    _same_run(on, off, KEYS, f"n = {n}: window on vs off")
    for k in KEYS:
        _bitwise(on[k], ref[k], f"n = {n} vs oracle: {k}")


@pytest.mark.parametrize("obs", ["negPhise0", True])
def test_obs_trajectory(rom, M, crossing, obs):
    """5. step_ex_obs reads the corner states of step t - 1 from the window: one slot and the full
    record across crossings and a flush; obs.Vcell is v."""
    c = crossing
    steps = 130
    on, off = (_run_obs(M, rom, c["soc0"], c["tc0"], c["tct"], env, obs, steps, c["cfg"]) for env in (ON, OFF))
    for k in KEYS:
        _bitwise(on[k], off[k], k)
        _bitwise(on[k], c["off"][k][:steps], f"{k} vs the call without obs")
    assert set(on["obs"]) == set(off["obs"])
    for k in on["obs"]:
        _bitwise(on["obs"][k], off["obs"][k], f"obs {k}")
    if obs is True:
        _bitwise(on["obs"]["Vcell"], on["v"], "obs.Vcell vs v")
    for k in STATE:
        _bitwise(on["state"][k], off["state"][k], f"state {k}")


@pytest.mark.parametrize("lookup", ["linear", "quintic"])
def test_lockout_and_error_cells(P, oc, M, lookup):
    """6. tests/test_gpu_parity.py test_lockout_and_error_cells' inputs: the plant is skipped for
    error cells, and the state after the call is the twin's."""
    rom = P.make_synth_rom(lookup=lookup)
    soc0 = np.array([10.0, 130.0, 20.0, 130.0])
    tc = np.array([25.0, 25.0, 15.0, 35.0])
    ref = oc.run(rom, soc0, tc, 70, nthreads=1)
    on, off = (_run(M, rom, soc0, tc, [70], env) for env in (ON, OFF))
    _same_run(on, off, KEYS, "window on vs off")
    assert (on["state"]["status"][[1, 3]] & 1).all()
    _bitwise(on["state"]["status"], ref["status"], "status vs oracle")
    for k in ("u", "v", "soc", "phise"):
        _bitwise(on[k], ref[k], f"vs oracle: {k}")


@pytest.mark.parametrize("axis", ["T", "SOC"])
def test_single_set_point_rom(P, oc, M, axis):
    """7. A ROM with one set-point on an axis: every cell's corners repeat, so no cell uses the
    window (the record path, tags left empty); equal to the twin and the oracle."""
    kw = dict(T_degC=(25.0,)) if axis == "T" else dict(SOC_pct=(50.0,))
    rom = P.make_synth_rom(lookup="quintic", **kw)
    soc0, tc = batch_inputs(100, seed=31)
    if axis == "T":
        soc0[:6] = rom.SOC_pct[2:8] - 0.05
    ref = oc.run(rom, soc0, tc, 80, nthreads=8)
    on, off = (_run(M, rom, soc0, tc, [80], env) for env in (ON, OFF))
    _same_run(on, off, KEYS, "window on vs off")
    for k in KEYS:
        _bitwise(on[k], ref[k], f"vs oracle: {k}")


def test_set_state_and_init_cells(rom, M, crossing):
    """8. set_state of a checkpoint taken mid-run, and init_cells on a used context: the window
    starts empty and the run goes on with the twin's bits."""
    c = crossing
    with _ctx(M, rom, N, ON, c["cfg"]) as a, _ctx(M, rom, N, OFF, c["cfg"]) as b:
        for x in (a, b):
            x.init_cells(c["soc0"], c["tc0"])
        ra, rb = (x.step(70, outputs=ZKEYS, tc=c["tct"][:70]) for x in (a, b))
        sa, sb = a.get_state(), b.get_state()
        for k in STATE:
            _bitwise(sa[k], sb[k], f"checkpoint: {k}")
        ra, rb = (x.step(30, outputs=ZKEYS, tc=c["tct"][70:100]) for x in (a, b))
        a.set_state(sa)
        b.set_state(sb)
        ra, rb = (x.step(70, outputs=ZKEYS, tc=c["tct"][70:140]) for x in (a, b))
        ta, tb = a.get_state(), b.get_state()
        for k in ZKEYS:
            _bitwise(ra[k], rb[k], f"after set_state: {k}")
            _bitwise(ra[k], c["off"][k][70:140], f"after set_state vs the uninterrupted run: {k}")
        for k in STATE:
            _bitwise(ta[k], tb[k], f"state after set_state: {k}")
        # the used contexts start again
        for x in (a, b):
            x.init_cells(c["soc0"], c["tc0"])
        ra, rb = (x.step(70, outputs=ZKEYS, tc=c["tct"][:70]) for x in (a, b))
        ta, tb = a.get_state(), b.get_state()
    for k in ZKEYS:
        _bitwise(ra[k], rb[k], f"after init_cells: {k}")
        _bitwise(ra[k], c["off"][k][:70], f"after init_cells vs a fresh context: {k}")
    for k in STATE:
        _bitwise(ta[k], tb[k], f"state after init_cells: {k}")
        _bitwise(ta[k], sa[k], f"state after init_cells vs the first 70 steps: {k}")


@pytest.mark.parametrize("route", ["graph", "np20", "switch_off", "split"])
def test_routes(rom, M, route):
    """9, 10. Graph replay (two calls of one shape), Np = 20 / Nc = 10 (64 cells x 80 steps) and
    the other forms of the fused step that run the plant in k_cell: window on == off."""
    n, steps = (64, 80) if route == "np20" else (136, 80)
    soc0, tc0, tct = crossing_inputs(rom, n, steps)
    cfg = {"np20": dict(Np=20, Nc=10), "switch_off": dict(constraints=(1, 0, 1))}.get(route, {})
    cfg = M.make_config(bounds=True, **cfg)
    extra = dict(MPCEKF_SPLIT_CELL=1) if route == "split" else {}
    chunks = [40, 40] if route == "graph" else [steps]   # the second call replays the captured graph
    on, off = (_run(M, rom, soc0, tc0, chunks, dict(env, **extra), cfg, tct, ZKEYS, graph=route == "graph")
               for env in (ON, OFF))
    _same_run(on, off, ZKEYS, route)


@pytest.mark.parametrize("kind", ["mb", "quad", "roll", "nm147"])
def test_contexts_without_a_plant_window(P, rom, M, kind):
    """11. Contexts that get no plant window run unchanged with the switch on."""
    n, steps = 136, 80
    if kind == "nm147":   # the model rows do not fit the LDS (rom_global): the plant runs as k_plant4
        rom = P.make_synth_rom(T_degC=tuple(np.linspace(15.0, 35.0, 7)), SOC_pct=tuple(np.linspace(0.0, 100.0, 21)))
        assert rom.NM == 147
        n = 65
    soc0, tc0, tct = crossing_inputs(rom, n, steps)
    cfg = M.make_config(bounds=True, **(dict(method="MB") if kind == "mb" else {}))
    extra = dict(mb={}, quad=dict(MPCEKF_QUAD=1), roll=dict(MPCEKF_FLUSH_ROLL=1), nm147={})[kind]
    on, off = (_run(M, rom, soc0, tc0, [steps], dict(env, **extra), cfg, tct, ZKEYS) for env in (ON, OFF))
    _same_run(on, off, ZKEYS, kind)


def test_step_summary(rom, M):
    """12a. step_summary across a flush window: the summary record and the state."""
    n, steps = 136, 80
    soc0, tc0, tct = crossing_inputs(rom, n, steps)
    res = []
    for env in (ON, OFF):
        with _ctx(M, rom, n, env) as ctx:
            ctx.init_cells(soc0, tc0)
            ctx.summary_begin(reach=0.2, obs="cellSOC")
            ctx.step_summary(steps, tc=tct)
            res.append((ctx.get_summary(), ctx.get_state()))
            ctx.summary_end()
    for k in res[0][0]:
        _bitwise(res[0][0][k], res[1][0][k], f"summary {k}")
    for k in STATE:
        _bitwise(res[0][1][k], res[1][1][k], f"state {k}")


def test_thermal_context(rom, M):
    """12b. A thermal context: the model drives the temperature through the 25 degC set-point."""
    n, steps = 136, 80
    soc0, _, _ = crossing_inputs(rom, n, steps)
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
