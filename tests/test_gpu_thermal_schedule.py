"""GPU: MPC limits scheduled over the thermal model's temperature inside the fused loop
(mpcekf_thermal_schedule / _schedule_end; k_sched before a call's first step, k_thermal_sched at
the end of every step another step follows).

What is compared with what:
  1. the host-driven loop: a thermal context without a schedule that, every step, reads T
     (thermal_get), evaluates include/mpcekf.h's lookup in numpy (sched_eval below), passes the
     values to set_limits and runs step(1).  That route is pinned to the C oracle by
     tests/test_gpu_limits.py and tests/test_gpu_thermal.py; the scheduled context must give its
     bits: u, v, soc, phise, nexec, temp, heat, get_limits, the thermal record, get_state;
  2. sched_eval itself against get_limits after each call of a one-step-per-call run;
  3. a constant schedule against uniform set_limits arrays and against a plain thermal context;
  4. a falling C-rate table against the bound it implies, and an unscheduled twin that breaks it;
  5. the scheduled context against itself across graph replay, step_summary and step_ex_obs.

Inputs (inputs() below; every property is asserted on the returned temp rows by check_inputs):
300 cells (a second, partial 256-thread block; a partial wave), at most 40 steps, the quintic
synthetic ROM.  Grid 20..40 degC, 5 knots (20, 25, 30, 35, 40).  T0 = 14 + 32 c / 299 for cell
c, so cells 0..56 start below T_lo, cells 243..299 above T_hi and the rest fill all four knot
intervals; then cell 3 is put exactly on T_lo, cell 4 exactly on T_hi, cell 5 exactly on the
knot 30.  Cth 20..100 J/K: at 2C a cell generates 6-18 W, i.e. several K over 40 steps, more than
one 5 K interval for the light cells.  Rth finite (2..6 K/W) on the even cells, +inf on the odd
ones, Tamb 15..30 degC.  Three derating maps, cell c on map perm[c] % 3 (a fixed shuffle).
Np = 20 / Nc = 10: the first 40 cells at stride 7 (so the spread of T0 stays) and 12 steps.
"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import summary_ref as sr
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

N = 300
CALLS = (7, 1, 32)
KEYS = ("u", "v", "soc", "phise", "nexec")
ROWS = KEYS + ("temp", "heat")
FIELDS = ("T", "T_max", "T_max_step", "T_min", "heat_sum", "steps", "nheld")
SCHED = ("Crate", "u_max", "du_min", "du_max", "v_max", "phise_min")
T_LO, T_HI, NTAB = 20.0, 40.0, 5
ST_ERROR = 1


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def inputs(n=N, stride=1):
    rng = np.random.Generator(np.random.PCG64(0x5C4ED))
    soc0, _ = batch_inputs(N)
    T0 = 14.0 + 32.0 * np.arange(N) / (N - 1)
    T0[3], T0[4], T0[5] = T_LO, T_HI, 30.0
    Cth = rng.uniform(20.0, 100.0, N)
    Rth = rng.uniform(2.0, 6.0, N)
    Rth[1::2] = np.inf
    sets = (rng.permutation(N) % 3).astype(np.int32)
    p = dict(soc0=soc0, T0=T0, Cth=Cth, Rth=Rth, Tamb=rng.uniform(15.0, 30.0, N), sets=sets)
    if (n, stride) != (N, 1):
        idx = np.r_[3, 4, 5, np.arange(6, N, stride)][:n]
        p = {k: np.ascontiguousarray(v[idx]) for k, v in p.items()}
    return p


def maps():
    """Three derating maps over the 5 knots: the C-rate falls as the cell warms, the plating
    margin rises when it is cold, v_max is lowered at the hot end."""
    crate = np.array([[2.0, 2.0, 1.6, 1.1, 0.5], [2.0, 1.8, 1.5, 1.0, 0.7], [1.5, 1.5, 1.5, 1.0, 0.5]])
    phise = np.array([[0.12, 0.10, 0.08, 0.08, 0.08], [0.14, 0.11, 0.09, 0.08, 0.07], [0.10, 0.10, 0.09, 0.08, 0.08]])
    vmax = np.array([[4.1, 4.1, 4.1, 4.05, 4.0], [4.1, 4.1, 4.08, 4.02, 3.95], [4.1, 4.1, 4.1, 4.1, 4.0]])
    return dict(Crate=crate, phise_min=phise, v_max=vmax)


def sched_eval(T, T_lo, T_hi, tab, sets=None):
    """include/mpcekf.h's lookup, one numpy operation per rounded fp64 operation, in its order.
    tab [ntab] or [nsets][ntab] -> the value of every cell."""
    tab = np.atleast_2d(np.asarray(tab, dtype=np.float64))
    ntab = tab.shape[1]
    row = tab[np.zeros(T.shape[0], dtype=int) if sets is None else sets]
    with np.errstate(all="ignore"):
        x = (T - T_lo) / (T_hi - T_lo)
        xc = np.where(x > 0.0, x, 0.0)
        xc = np.where(xc < 1.0, xc, 1.0)
        s = xc * float(ntab - 1)
        j = np.minimum(s.astype(np.int64), ntab - 2)
        f = s - j.astype(np.float64)
        c = np.arange(T.shape[0])
        return row[c, j] + f * (row[c, j + 1] - row[c, j])


def interval(T):
    """The knot interval of the main grid a temperature falls into: -1 below, 4 above."""
    return np.where(T < T_LO, -1, np.where(T > T_HI, NTAB - 1, np.minimum(((T - T_LO) / 5.0).astype(int), NTAB - 2)))


def check_inputs(temp):
    """The properties the module docstring promises, on the temperatures the steps used."""
    iv = interval(temp)
    assert (temp[0] < T_LO).any() and (temp[0] > T_HI).any(), "both clamps from step 1"
    assert len(set(iv[0][(iv[0] >= 0) & (iv[0] < NTAB - 1)].tolist())) >= 3, "three knot intervals at step 1"
    assert (iv[-1] != iv[0]).any(), "some cell changes its knot interval during the run"


def state_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if a[k].dtype.kind == "f":
            sr.bits_equal(a[k], b[k], f"{what}: state {k}")
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: state {k}"


def same(a, b, what):
    """Equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if not eq.all():
        i = tuple(np.argwhere(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {a.size} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def begin(M, rom, ctx, p, status=None):
    ctx.init_cells(p["soc0"], p["T0"])
    if status is not None:
        st = ctx.get_state()
        st["status"] = status
        ctx.set_state(st)
    ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))


def collect(ctx, parts):
    out = {k: np.concatenate([q[k] for q in parts]) for k in ROWS} if parts else {}
    out.update(limits=ctx.get_limits(), rec=ctx.thermal_get(), state=ctx.get_state())
    return out


def run_scheduled(M, rom, p, calls, tabs, cfg=None, sets=True, graph=False, status=None):
    """Context A: the schedule inside the fused calls."""
    with M.Context(rom, p["soc0"].shape[0], cfg) as ctx:
        begin(M, rom, ctx, p, status)
        ctx.set_graph(graph)
        ctx.thermal_schedule(T_LO, T_HI, sets=p["sets"] if sets else None, **tabs)
        return collect(ctx, [ctx.step(m, outputs=KEYS, thermal=("temp", "heat")) for m in calls])


def run_host_driven(M, rom, p, nsteps, tabs, cfg=None, sets=True):
    """Context B: no schedule; every step reads T, evaluates the lookup in numpy, set_limits, step(1)."""
    with M.Context(rom, p["soc0"].shape[0], cfg) as ctx:
        begin(M, rom, ctx, p)
        parts = []
        for _ in range(nsteps):
            T = ctx.thermal_get("T")["T"]
            ctx.set_limits(**{k: sched_eval(T, T_LO, T_HI, t, p["sets"] if sets else None) for k, t in tabs.items()})
            parts.append(ctx.step(1, outputs=KEYS, thermal=("temp", "heat")))
        return collect(ctx, parts)


def compare(a, b, what):
    for k in ROWS:
        same(a[k], b[k], f"{what}: {k}")
    for k in a["limits"]:
        sr.bits_equal(a["limits"][k], b["limits"][k], f"{what}: get_limits {k}")
    for k in FIELDS:
        sr.bits_equal(a["rec"][k], b["rec"][k], f"{what}: record {k}")
    state_equal(a["state"], b["state"], what)


@pytest.fixture(scope="module")
def ctx_a(M, rom):
    """Test 1's context A at Np = 5 / Nc = 2, every switch on (shared, read-only)."""
    return run_scheduled(M, rom, inputs(), CALLS, maps())


# ---- 1. parity with the host-driven loop, bit for bit -----------------------------------------
@pytest.mark.parametrize("arm", ["np5_111", "np5_110", "wide", "mb"])
def test_parity_with_host_driven_loop(M, rom, ctx_a, arm):
    kw = dict(np5_111={}, np5_110=dict(constraints=(1, 1, 0)), wide=dict(Np=20, Nc=10), mb=dict(method="MB"))[arm]
    p, calls = (inputs(40, 7), (7, 1, 4)) if arm == "wide" else (inputs(), CALLS)
    cfg = M.make_config(**kw)
    a = ctx_a if arm == "np5_111" else run_scheduled(M, rom, p, calls, maps(), cfg)
    check_inputs(a["temp"])
    sr.bits_equal(a["temp"][0], p["T0"], "temp[0] is T0")
    assert {T_LO, T_HI, 30.0} <= set(a["temp"][0].tolist()), "cells exactly on T_lo, on T_hi and on a knot"
    assert set(p["sets"].tolist()) == {0, 1, 2}
    b = run_host_driven(M, rom, p, sum(calls), maps(), cfg)
    compare(a, b, arm)
    # the values in force after the call are those its last step used
    for k, t in maps().items():
        sr.bits_equal(a["limits"][k], sched_eval(a["temp"][-1], T_LO, T_HI, t, p["sets"]), f"{arm}: limits {k}")
    assert np.isfinite(a["u"]).all() and (a["state"]["status"] == 0).all()


# ---- 2. the recurrence restated ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["ntab2", "nsets3"])
def test_recurrence_restated(M, rom, case):
    """get_limits after each call of a one-step-per-call run is sched_eval at that step's temp
    row: T exactly at T_lo (cell 3), at T_hi (cell 4) and on a knot (cell 5) at step 1; ntab = 2
    (one interval, j = 0 everywhere); nsets = 3 with the shuffled set_of_cell."""
    p = inputs()
    tabs = dict(Crate=np.array([2.0, 0.5]), du_max=np.array([50.0, 20.0])) if case == "ntab2" else maps()
    sets = p["sets"] if case == "nsets3" else None
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p)
        ctx.thermal_schedule(T_LO, T_HI, sets=sets, **tabs)
        # set at once: the values at the temperatures as they stand
        for k, t in tabs.items():
            sr.bits_equal(ctx.get_limits()[k], sched_eval(p["T0"], T_LO, T_HI, t, sets), f"at set: {k}")
        temps = []
        for step in range(8):
            o = ctx.step(1, outputs=("u",), thermal="temp")
            temps.append(o["temp"][0])
            lim = ctx.get_limits()
            for k, t in tabs.items():
                sr.bits_equal(lim[k], sched_eval(o["temp"][0], T_LO, T_HI, t, sets), f"step {step}: {k}")
            if step == 0:
                assert o["temp"][0, 3] == T_LO and o["temp"][0, 4] == T_HI and o["temp"][0, 5] == 30.0
                for k, t in tabs.items():   # f = 0 at T_lo and on a knot: the table entry itself
                    rows = np.atleast_2d(t)[[0, 0] if sets is None else sets[[3, 5]]]
                    assert lim[k][3] == rows[0, 0]
                    if case == "nsets3":
                        assert lim[k][5] == rows[1, 2]
            # unscheduled fields: the configuration's scalars
            assert (lim["z_max"] == 0.95).all() and (lim["target_soc"] == 95.0).all()
        temps = np.array(temps)
        assert (temps[0] < T_LO).any() and (temps[0] > T_HI).any() and (temps[-1] != temps[0]).any()


# ---- 3. a constant table changes nothing ------------------------------------------------------
def test_constant_schedule_changes_nothing(M, rom):
    p = inputs()
    cfg = M.make_config()
    const = {k: float(getattr(cfg, k)) for k in SCHED}
    tabs = {k: np.full((3, NTAB), v) for k, v in const.items()}
    a = run_scheduled(M, rom, p, CALLS, tabs)
    check_inputs(a["temp"])
    with M.Context(rom, N) as ctx:                      # the same fields as uniform set_limits arrays
        begin(M, rom, ctx, p)
        ctx.set_limits(**{k: np.full(N, v) for k, v in const.items()})
        b = collect(ctx, [ctx.step(m, outputs=KEYS, thermal=("temp", "heat")) for m in CALLS])
    with M.Context(rom, N) as ctx:                      # a plain thermal context
        begin(M, rom, ctx, p)
        c = collect(ctx, [ctx.step(m, outputs=KEYS, thermal=("temp", "heat")) for m in CALLS])
    compare(a, b, "uniform set_limits")
    compare(a, c, "plain thermal context")


# ---- 4. it does something ---------------------------------------------------------------------
def test_falling_crate_binds(M, rom, ctx_a):
    p = inputs()
    Q = float(rom.Q)
    tabs = dict(Crate=np.linspace(2.0, 0.5, NTAB))
    a = run_scheduled(M, rom, p, (40,), tabs, sets=False)
    with M.Context(rom, N) as ctx:                      # the unscheduled twin
        begin(M, rom, ctx, p)
        b = ctx.step(40, outputs=KEYS, thermal=("temp", "heat"))
    hot_a, hot_b = a["temp"] >= T_HI, b["temp"] >= T_HI
    assert hot_a[0].sum() >= 50 and hot_a.any(axis=0).sum() > hot_a[0].sum(), "cells start above T_hi and heat past it mid-run"
    print("min over hot cell-steps of u + Q/2:", float((a["u"][hot_a] + Q * 0.5).min()))
    assert (a["u"][hot_a] >= -Q * 0.5 - 1e-9).all()
    assert (b["u"][hot_b] < -Q * 0.5 - 1e-9).any()


# ---- 5. T changed between calls ---------------------------------------------------------------
def test_temperature_changed_between_calls(M, rom):
    p = inputs()
    tabs = maps()
    rng = np.random.Generator(np.random.PCG64(7))
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p)
        ctx.thermal_schedule(T_LO, T_HI, sets=p["sets"], **tabs)
        ctx.step(3, outputs=())
        for how in ("stage", "begin"):
            Tn = rng.permutation(p["T0"])              # every cell somewhere else on (and off) the grid
            if how == "stage":
                ctx.OB_step(ctx.get_scalars(("uk",))["uk"], Tc=Tn)   # a stage call's temperature argument
            else:
                ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom), T0=Tn)
            o = ctx.step(1, outputs=("u",), thermal="temp")
            sr.bits_equal(o["temp"][0], Tn, f"{how}: temp[0]")
            lim = ctx.get_limits()
            for k, t in tabs.items():
                sr.bits_equal(lim[k], sched_eval(Tn, T_LO, T_HI, t, p["sets"]), f"{how}: {k}")
            o = ctx.step(2, outputs=("u",), thermal="temp")             # and on: the model's own T again
            for k, t in tabs.items():
                sr.bits_equal(ctx.get_limits()[k], sched_eval(o["temp"][-1], T_LO, T_HI, t, p["sets"]), f"{how} + 2: {k}")


# ---- 6. held and error cells ------------------------------------------------------------------
def test_held_and_error_cells(M, rom, ctx_a):
    held, bad = 7, 130
    p = inputs()
    p["Cth"][held] = 1e-3                              # J/K: any charging step overshoots 100 degC
    status = np.zeros(N, dtype=np.int32)
    status[bad] = ST_ERROR
    a = run_scheduled(M, rom, p, CALLS, maps(), status=status)
    rec, temp = a["rec"], a["temp"]
    assert rec["nheld"][held] >= 38 and (temp[5:, held] == temp[5, held]).all()
    assert rec["nheld"][bad] == 40 and (temp[:, bad] == p["T0"][bad]).all()
    assert np.isnan(a["u"][:, bad]).all() and np.isnan(a["v"][:, bad]).all() and np.isnan(a["heat"][:, bad]).all()
    for k, t in maps().items():
        want = sched_eval(temp[-1], T_LO, T_HI, t, p["sets"])
        sr.bits_equal(a["limits"][k], want, f"limits {k}")
        assert np.isfinite(a["limits"][k][[held, bad]]).all()
        assert a["limits"][k][held] == sched_eval(temp[5], T_LO, T_HI, t, p["sets"])[held]     # held T, kept limits
        assert a["limits"][k][bad] == sched_eval(p["T0"], T_LO, T_HI, t, p["sets"])[bad]
    keep = ~np.isin(np.arange(N), (held, bad))
    for k in ("u", "temp"):
        same(a[k][:, keep], ctx_a[k][:, keep], f"neighbours: {k}")


# ---- 7. routes (the scheduled context against itself) -----------------------------------------
@pytest.mark.parametrize("route", ["graph", "graph_1x40", "summary", "obs"])
def test_routes(M, rom, ctx_a, route):
    p = inputs()
    if route in ("graph", "graph_1x40"):                # 1x40: one captured shape replayed 39 times
        a = run_scheduled(M, rom, p, CALLS if route == "graph" else (1,) * 40, maps(), graph=True)
        compare(a, ctx_a, route)
        return
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p)
        ctx.thermal_schedule(T_LO, T_HI, sets=p["sets"], **maps())
        if route == "summary":
            ctx.summary_begin()
            for m in CALLS:
                ctx.step_summary(m)
            s = ctx.get_summary()
            sr.bits_equal(s["u_last"], ctx_a["u"][-1], "summary: u_last")
            sr.bits_equal(s["u_min"], ctx_a["u"].min(axis=0), "summary: u_min")
        else:
            parts = [ctx.step(m, outputs=KEYS, obs=("negSOC",)) for m in CALLS]        # mpcekf_step_ex_obs, one slot
            for k in KEYS:
                same(np.concatenate([q[k] for q in parts]), ctx_a[k], f"obs: {k}")
        got = collect(ctx, [])
    for k in got["limits"]:
        sr.bits_equal(got["limits"][k], ctx_a["limits"][k], f"{route}: get_limits {k}")
    for k in FIELDS:
        sr.bits_equal(got["rec"][k], ctx_a["rec"][k], f"{route}: record {k}")
    state_equal(got["state"], ctx_a["state"], route)


def test_schedule_replaced_between_replays(M, rom):
    """Graph replay on: three replays under one schedule, then another schedule of the same
    shape (the same buffers: the captured graph is replayed) and one of another shape; a twin
    without graphs does the same."""
    p = inputs()
    second = {k: v[::-1].copy() for k, v in maps().items()}                 # the maps in another order
    third = dict(Crate=np.linspace(2.0, 0.5, 33), du_min=np.linspace(-50.0, -10.0, 33))   # larger tables: regrown

    def run(graph):
        with M.Context(rom, N) as ctx:
            begin(M, rom, ctx, p)
            ctx.set_graph(graph)
            parts = []
            for tabs, sets in ((maps(), p["sets"]), (second, p["sets"]), (third, None)):
                ctx.thermal_schedule(T_LO, T_HI + (5.0 if tabs is third else 0.0), sets=sets, **tabs)
                parts += [ctx.step(1, outputs=KEYS, thermal=("temp", "heat")) for _ in range(4)]
            return collect(ctx, parts), parts
    (a, pa), (b, _) = run(True), run(False)
    compare(a, b, "replaced schedule under graph replay")
    assert not np.array_equal(a["u"][4:8], run_scheduled(M, rom, p, (8,), maps())["u"][4:8]), "the second schedule is in force"
    assert (a["limits"]["phise_min"] == 0.08).all()                         # the third schedule dropped the field
    sr.bits_equal(a["limits"]["du_min"], sched_eval(a["temp"][-1], T_LO, T_HI + 5.0, third["du_min"]), "third: du_min")


# ---- 8. refusals on a live context ------------------------------------------------------------
def test_refusals_on_a_live_context(M, rom):
    n = 7
    p = inputs(n, 45)
    tabs = maps()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tab = np.ascontiguousarray(np.stack([tabs["Crate"], tabs["phise_min"]], axis=1))   # [3][2][5]
    ids = lambda *x: np.array(x, dtype=np.int32)
    F = ids(1, 6)                                                                      # CRATE, PHISE_MIN

    def put(i, v):
        b = tab.copy()
        b.flat[i] = v
        return b

    def refused(ctx):
        L, h = ctx.L, ctx.h
        I = lambda a: None if a is None else a.ctypes.data_as(ip)
        D = lambda a: None if a is None else a.ctypes.data_as(dp)
        s_bad, s_neg = p["sets"].copy(), p["sets"].copy()
        s_bad[4], s_neg[2] = 3, -1
        for args, msg in (((2, None, 5, T_LO, T_HI, 3, D(tab), I(p["sets"])), b"null fields"),
                          ((2, I(F), 5, T_LO, T_HI, 3, None, I(p["sets"])), b"null tables"),
                          ((0, I(F), 5, T_LO, T_HI, 3, D(tab), None), b"nfields = 0 outside 1..6"),
                          ((7, I(ids(*range(7))), 5, T_LO, T_HI, 3, D(tab), None), b"nfields = 7 outside 1..6"),
                          ((2, I(ids(1, 1)), 5, T_LO, T_HI, 3, D(tab), None), b"id 1 given twice"),
                          ((2, I(ids(1, 0)), 5, T_LO, T_HI, 3, D(tab), None), b"fields[1] = 0 cannot be scheduled"),
                          ((2, I(ids(7, 1)), 5, T_LO, T_HI, 3, D(tab), None), b"fields[0] = 7 cannot be scheduled"),
                          ((2, I(ids(1, 8)), 5, T_LO, T_HI, 3, D(tab), None), b"fields[1] = 8 cannot be scheduled"),
                          ((2, I(ids(1, 9)), 5, T_LO, T_HI, 3, D(tab), None), b"fields[1] = 9 cannot be scheduled"),
                          ((2, I(F), 1, T_LO, T_HI, 3, D(tab), None), b"ntab = 1"),
                          ((2, I(F), 5, np.nan, T_HI, 3, D(tab), None), b"grid [nan, 40]"),
                          ((2, I(F), 5, T_LO, np.inf, 3, D(tab), None), b"grid [20, inf]"),
                          ((2, I(F), 5, T_LO, T_LO, 3, D(tab), None), b"grid [20, 20]"),
                          ((2, I(F), 5, T_HI, T_LO, 3, D(tab), None), b"grid [40, 20]"),
                          ((2, I(F), 5, T_LO, T_HI, 3, D(put(13, np.nan)), None), b"tables[13] = nan"),
                          ((2, I(F), 5, T_LO, T_HI, 3, D(put(29, -np.inf)), None), b"tables[29] = -inf"),
                          ((2, I(F), 5, T_LO, T_HI, 0, D(tab), None), b"nsets = 0"),
                          ((2, I(F), 5, T_LO, T_HI, 3, D(tab), I(s_bad)), b"set_of_cell[4] = 3 outside 0..2"),
                          ((2, I(F), 5, T_LO, T_HI, 3, D(tab), I(s_neg)), b"set_of_cell[2] = -1 outside 0..2")):
            assert L.mpcekf_thermal_schedule(h, *args) == -1, msg
            assert msg in L.mpcekf_last_error(), (msg, L.mpcekf_last_error())
        assert L.mpcekf_thermal_schedule(None, 2, I(F), 5, T_LO, T_HI, 3, D(tab), None) == -1

    sub = dict(Crate=tabs["Crate"], phise_min=tabs["phise_min"])
    with M.Context(rom, n) as ctx, M.Context(rom, n) as twin, M.Context(rom, n) as plain:
        for c in (ctx, twin, plain):
            c.init_cells(p["soc0"], p["T0"])
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_schedule: call mpcekf_thermal_begin first"):
            ctx.thermal_schedule(T_LO, T_HI, **sub)
        ctx.thermal_schedule_end()                                    # a no-op without a schedule
        for c in (ctx, twin, plain):
            c.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))
        refused(ctx)                                                  # on a context without a schedule: none begins
        assert (ctx.get_limits()["Crate"] == 2.0).all()
        for c in (ctx, twin):
            c.thermal_schedule(T_LO, T_HI, sets=p["sets"], **sub)
            c.step(5, outputs=())
        refused(ctx)                                                  # on a context with one: it stays
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: set_limits: .* is scheduled over temperature"):
            ctx.set_limits(v_max=4.0, Crate=1.0)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: clear_limits: a temperature schedule is active"):
            ctx.clear_limits()
        for k, v in twin.get_limits().items():
            sr.bits_equal(ctx.get_limits()[k], v, f"after refusals: get_limits {k}")
        for c in (ctx, twin):
            c.set_limits(v_max=np.linspace(4.0, 4.1, n))               # an unscheduled field may be set
        a, b = (c.step(6, outputs=KEYS, thermal=("temp", "heat")) for c in (ctx, twin))
        for k in ROWS:
            same(a[k], b[k], f"after refusals: {k}")
        state_equal(ctx.get_state(), twin.get_state(), "after refusals")
        assert (ctx.get_limits()["Crate"] != 2.0).any()
        # schedule_end: the fields back to what set_limits / the configuration gave; v_max stays set
        ctx.thermal_schedule_end()
        lim = ctx.get_limits()
        assert (lim["Crate"] == 2.0).all() and (lim["phise_min"] == 0.08).all()
        sr.bits_equal(lim["v_max"], np.linspace(4.0, 4.1, n), "v_max after schedule_end")
        plain.set_state(ctx.get_state())
        plain.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom), T0=ctx.thermal_get("T")["T"])
        plain.set_limits(v_max=np.linspace(4.0, 4.1, n))
        a, b = (c.step(6, outputs=KEYS, thermal=("temp", "heat")) for c in (ctx, plain))
        for k in ROWS:
            same(a[k], b[k], f"after schedule_end: {k}")
        ctx.clear_limits()                                             # allowed again
        # thermal_end drops the schedule
        twin.thermal_end()
        assert (twin.get_limits()["Crate"] == 2.0).all()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_schedule"):
            twin.thermal_schedule(T_LO, T_HI, **sub)
        twin.clear_limits()
        assert (twin.get_limits()["v_max"] == 4.1).all()


def test_wrappers_pass_the_schedule_through(M, rom, ctx_a):
    p, n, steps = inputs(), 9, 8
    th = dict(Cth=p["Cth"][:n], Rth=p["Rth"][:n], Tamb=p["Tamb"][:n], ocv=M.thermal_ocv(rom),
              schedule=dict(T_lo=T_LO, T_hi=T_HI, sets=p["sets"][:n], **maps()))
    out = M.runMPC(rom, p["soc0"][:n], p["T0"][:n], steps, thermal=th)
    for k in ("u", "v", "temp", "heat"):
        same(out[k], ctx_a[k][:steps, :n], f"runMPC: {k}")
    for k, t in maps().items():
        sr.bits_equal(out["limits"][k], sched_eval(out["temp"][-1], T_LO, T_HI, t, p["sets"][:n]), f"runMPC: limits {k}")
    s = M.run_summary(rom, p["soc0"][:n], p["T0"][:n], steps, thermal=th, chunk=3)
    sr.bits_equal(s["u_last"], out["u"][-1], "run_summary: u_last")
    sr.bits_equal(s["thermal"]["T"], out["thermal"]["T"], "run_summary: T")
