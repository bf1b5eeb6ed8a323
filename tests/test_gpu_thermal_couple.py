"""GPU: heat conduction between neighbouring cells of a pack string along the fused loop
(mpcekf_thermal_couple / _couple_get / _couple_end, mpcekf_step_ex_couple; k_thermal_couple and
k_thermal_couple_sched in k_thermal's and k_thermal_sched's place, k_couple_seed once per call).

What is compared with what:
  1. tests/couple_ref.py, the numpy restatement of include/mpcekf.h's rule, driven by the GPU's
     own u (shifted one step), v and the plant's negSOC: temp, heat, cond, the thermal record
     and the coupling's record bit for bit (a NaN equals a NaN);
  2. the C oracle fed the temperatures the model produced, and the host-driven loop: a pack
     context with the uncoupled model stepped once per step, its temperature replaced before
     every step by the one the numpy rule gives.  The oracle knows no strings: it gives every
     cell's own command, so its rows can equal the pack's only up to the first step at which a
     string's current differs from a cell's command; the comparison runs up to that step per
     string, and the host-driven loop carries the comparison over every step;
  3. the coupled context against itself: odd call splits (the snapshot's parity flips), graph
     replay, step_summary, outputs on the device, a second identical run;
  4. with a schedule: the host-driven loop of tests/test_gpu_thermal_schedule.py on a coupled
     context;
  5. identity: S = 1, every link +inf, and after thermal_couple_end, against a thermal pack
     context that never had links;
  6. a stage call's temperature argument and a fresh init_cells between two fused calls;
  7. a cell in error: its T is held and its neighbours still conduct;
  8. S = 2: the two flows over a link cancel exactly;
  9. refusals change nothing.
Nothing expected comes from the code under test except where a test says "against itself".

Shapes: 260 cells with S = 13 (20 strings; string 4 straddles the wave boundary at lane 64,
string 19 the 256-thread block boundary), S = 2, S = 260 and S = 1; 70 steps (across the 64-step
flush period and the summary window); Np = 20 / Nc = 10: 24 cells, S = 4, 12 steps.
"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import couple_ref as cr
import summary_ref as sr
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

N, S, STEPS = 260, 13, 70
KEYS = ("u", "v", "soc", "phise", "nexec")
ROWS = KEYS + ("temp", "heat", "cond", "ucmd")
FIELDS = cr.THERMAL_FIELDS
CFIELDS = cr.COUPLE_FIELDS
ST_ERROR = 1


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")   # set-points 15 / 25 / 35 degC


def params(n, seed=0x7E44):
    """tests/test_gpu_thermal.py's per-cell parameters (Cth 40..160 J/K, Rth 2..6 K/W on the even
    cells and +inf on the odd ones, Tamb 15..30 degC, T0 24..29 degC: neighbours start up to 5 K
    apart), plus the links: 0.5..5 K/W, every fifth one +inf."""
    rng = np.random.Generator(np.random.PCG64(seed))
    soc0, _ = batch_inputs(n)
    Cth = rng.uniform(40.0, 160.0, n)
    Rth = rng.uniform(2.0, 6.0, n)
    Rth[1::2] = np.inf
    p = dict(soc0=soc0, T0=rng.uniform(24.0, 29.0, n), Cth=Cth, Rth=Rth, Tamb=rng.uniform(15.0, 30.0, n))
    p["links"] = rng.uniform(0.5, 5.0, n)
    p["links"][4::5] = np.inf
    return p


def same(a, b, what=""):
    """Equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if not eq.all():
        i = tuple(np.argwhere(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {a.size} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def state_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if a[k].dtype.kind == "f":
            sr.bits_equal(a[k], b[k], f"{what}: state {k}")
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: state {k}"


def begin(M, rom, ctx, p, series, status=None, links=True, graph=False):
    ctx.init_cells(p["soc0"], p["T0"])
    if status is not None:
        st = ctx.get_state()
        st["status"] = status
        ctx.set_state(st)
    ctx.set_graph(graph)
    ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))
    ctx.pack_begin(series)
    if links:
        ctx.thermal_couple(p["links"])


def collect(ctx, parts, coupled=True):
    rows = ROWS if coupled else tuple(k for k in ROWS if k != "cond")
    out = {k: np.concatenate([q[k] for q in parts]) for k in rows} if parts else {}
    if parts:
        out["negSOC"] = np.concatenate([q["obs"]["negSOC"] for q in parts])
    out.update(rec=ctx.thermal_get(), pack=ctx.pack_get(), state=ctx.get_state(),
               socn_end=ctx.get_scalars(("SOCnAvg",))["SOCnAvg"].copy())
    if coupled:
        out["crec"] = ctx.thermal_couple_get()
    return out


def run_coupled(M, rom, n, series, calls, cfg=None, p=None, status=None, graph=False, summary=False, links=True):
    """A thermal pack context with links over the calls' steps: trajectories (none with
    summary=True), the records, the state, the current before the first step."""
    p = p or params(n)
    with M.Context(rom, n, cfg) as ctx:
        begin(M, rom, ctx, p, series, status, links, graph)
        uk0 = ctx.get_scalars(("uk",))["uk"].copy()
        th = ("temp", "heat", "cond") if links else ("temp", "heat")
        parts = []
        if summary:
            ctx.summary_begin()
        for m in calls:
            if summary:
                ctx.step_summary(m)
            else:
                parts.append(ctx.step(m, outputs=KEYS, obs=("negSOC",), thermal=th, pack=("ucmd",)))
        out = collect(ctx, parts, links)
        if summary:
            out["summary"] = ctx.get_summary()
        out.update(uk0=uk0, p=p, series=series, ocv=M.thermal_ocv(rom))
    return out


def restate(rom, g, status=None):
    p = g["p"]
    err = None if status is None else (status & ST_ERROR) != 0
    return cr.restate(float(rom.Ts), float(rom.neg.theta0), float(rom.neg.theta100), p, g["ocv"], p["links"], g["series"],
                      p["T0"], g["uk0"], g["u"], g["v"], g["negSOC"], g["socn_end"], error=err)


def check_restated(rom, g, what, status=None):
    temp, heat, cond, th, cp = restate(rom, g, status)
    sr.bits_equal(temp, g["temp"], f"{what}: temp")
    same(heat, g["heat"], f"{what}: heat")
    same(cond, g["cond"], f"{what}: cond")
    assert tuple(g["rec"]) == FIELDS and tuple(g["crec"]) == CFIELDS
    for k in FIELDS:
        sr.bits_equal(g["rec"][k], th[k], f"{what}: thermal record {k}")
    for k in CFIELDS:
        same(g["crec"][k], cp[k], f"{what}: coupling record {k}")
    return temp, heat, cond, th, cp


def compare(a, b, what, rows=ROWS):
    for k in rows:
        same(a[k], b[k], f"{what}: {k}")
    for k in FIELDS:
        sr.bits_equal(a["rec"][k], b["rec"][k], f"{what}: thermal record {k}")
    for k in a["pack"]:
        sr.bits_equal(a["pack"][k], b["pack"][k], f"{what}: pack record {k}")
    if "crec" in a and "crec" in b:
        for k in CFIELDS:
            same(a["crec"][k], b["crec"][k], f"{what}: coupling record {k}")
    state_equal(a["state"], b["state"], what)


@pytest.fixture(scope="module")
def base(M, rom):
    """260 cells, S = 13, 70 steps in one call (shared, read-only)."""
    return run_coupled(M, rom, N, S, (STEPS,))


# ---- 1. the rule, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["np5", "np5_mb", "wide", "wide_mb", "S2", "S260"])
def test_rule_bitwise(M, rom, base, arm):
    kw = dict(np5={}, np5_mb=dict(method="MB"), wide=dict(Np=20, Nc=10), wide_mb=dict(Np=20, Nc=10, method="MB"),
              S2={}, S260={})[arm]
    n, series, steps = (24, 4, 12) if arm.startswith("wide") else (N, dict(S2=2, S260=N).get(arm, S), STEPS)
    g = base if arm == "np5" else run_coupled(M, rom, n, series, (steps,), M.make_config(**kw) if kw else None)
    temp, heat, cond, th, cp = check_restated(rom, g, arm)
    # the floors: conduction did something, in both directions, and not over the missing links
    pos = np.arange(n) % series
    nl = ((pos > 0) & np.isfinite(np.roll(g["p"]["links"], 1))).astype(int) + \
         ((pos < series - 1) & np.isfinite(g["p"]["links"])).astype(int)
    assert ((nl == 2).any() or series == 2) and (nl == 1).any() and ((nl == 0).any() or series == N)
    assert (cond[:, nl > 0] != 0).all(axis=0).any() and (cond > 0).any() and (cond < 0).any()
    assert (cond[:, nl == 0] == 0).all() and not np.signbit(cond[:, nl == 0]).any()
    assert (cp["DT_MAX"][nl > 0] > 0.5).any() and np.isnan(cp["DT_MAX"][nl == 0]).all()
    assert (th["steps"] == steps).all()
    if arm == "np5":
        assert (cp["DT_MAX_STEP"] > 1).any(), "some gradient peaks after the first step"
        for b in (64, 256):       # a string across the wave boundary and one across the block boundary
            assert pos[b] > 0 and np.isfinite(g["p"]["links"][b - 1]) and (cond[:, b] != 0).all()


# ---- 2. the oracle given the temperatures, and the host-driven loop ---------------------------
def test_oracle_given_the_temperatures(M, rom, oc, base):
    p, n = base["p"], N
    ref = oc.run(rom, p["soc0"], p["T0"], STEPS, nthreads=8, tc_traj=base["temp"])
    # the first step at which some cell of the string did not get its own command: up to and
    # including it every cell has seen only its own commands, as the oracle's cells do
    own = (base["ucmd"].view(np.uint64) == base["u"].view(np.uint64)).reshape(STEPS, n // S, S).all(axis=2)
    first = np.where(own.all(axis=0), STEPS - 1, np.argmin(own, axis=0))
    upto = np.repeat(first, S)
    for k in KEYS:
        got = base["ucmd"] if k == "u" else base[k]
        for t in range(int(upto.max()) + 1):
            c = upto >= t
            same(got[t, c].astype(np.float64), ref[k][t, c].astype(np.float64), f"oracle: {k} of step {t}")
    assert (ref["status"] == 0).all()
    print("oracle: steps compared per string:", (first + 1).tolist())


def test_host_driven_loop(M, rom, base):
    """The round trip the coupling replaces: a pack context with the uncoupled model, step(1),
    and before every step the temperature the numpy rule gives (temp[k] of the restatement, set
    through thermal_begin's t0)."""
    p = base["p"]
    temp, _, _, th, _ = restate(rom, base)
    ocv = M.thermal_ocv(rom)
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p, S, links=False)
        for k in range(STEPS):
            ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], ocv, T0=temp[k])
            o = ctx.step(1, outputs=KEYS, pack=("ucmd",))
            for f in KEYS + ("ucmd",):
                same(o[f][0].astype(np.float64), base[f][k].astype(np.float64), f"{f} of step {k}")
        ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], ocv, T0=th["T"])    # the temperature the last step leaves
        state_equal(ctx.get_state(), base["state"], "host-driven loop")


# ---- 3. the coupled context against itself -----------------------------------------------------
@pytest.mark.parametrize("how", ["1+5+64", "graph_1+5+64", "graph_70x1", "summary", "again"])
def test_against_itself(M, rom, base, how):
    calls = {"1+5+64": (1, 5, 64), "graph_1+5+64": (1, 5, 64), "graph_70x1": (1,) * STEPS, "summary": (66, 4),
             "again": (STEPS,)}[how]
    got = run_coupled(M, rom, N, S, calls, graph=how.startswith("graph"), summary=how == "summary")
    compare(got, base, how, rows=() if how == "summary" else ROWS)
    if how == "summary":
        sr.same_record(got["summary"], sr.reduce(base), how, fields=[k for k in sr.FIELDS if not k.startswith("obs_")])


def test_outputs_on_the_device(M, rom, base):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    p = base["p"]
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p, S)
        bufs = {k: M.DeviceBuffer((STEPS, N), np.int32 if k == "nexec" else np.float64) for k in ROWS}
        try:
            tr = lib.Traj()
            at = 0
            for m in (3, 67):      # the second call's rows start at an odd row: the parity is the call's own
                off = lambda k: C.c_void_p(bufs[k].ptr + at * bufs[k].row_bytes())
                for k in KEYS:
                    setattr(tr, k, off(k).value)
                lib.check(ctx.L.mpcekf_step_ex_couple(ctx.h, m, None, C.byref(tr), None, 0, None, off("temp"), off("heat"),
                                                      off("ucmd"), None, None, off("cond"), 1))
                at += m
            ctx.sync()
            for k in ROWS:
                same(bufs[k].to_host().astype(np.float64), base[k].astype(np.float64), f"device: {k}")
        finally:
            for b in bufs.values():
                b.free()
        for k in CFIELDS:
            same(ctx.thermal_couple_get()[k], base["crec"][k], f"device: coupling record {k}")


# ---- 4. with a schedule that binds -------------------------------------------------------------
def sched_eval(T, T_lo, T_hi, tab):
    """include/mpcekf.h's lookup (tests/test_gpu_thermal_schedule.py), one table for every cell."""
    tab = np.asarray(tab, dtype=np.float64)
    ntab = tab.shape[0]
    with np.errstate(all="ignore"):
        x = (T - T_lo) / (T_hi - T_lo)
        xc = np.where(x > 0.0, x, 0.0)
        xc = np.where(xc < 1.0, xc, 1.0)
        s = xc * float(ntab - 1)
        j = np.minimum(s.astype(np.int64), ntab - 2)
        f = s - j.astype(np.float64)
        return tab[j] + f * (tab[j + 1] - tab[j])


def test_schedule_on_a_coupled_context(M, rom, base):
    steps, T_lo, T_hi = 40, 24.0, 32.0
    tabs = dict(Crate=np.linspace(2.0, 0.4, 5), phise_min=np.array([0.12, 0.10, 0.09, 0.08, 0.08]))
    p = base["p"]
    th = ("temp", "heat", "cond")
    with M.Context(rom, N) as a, M.Context(rom, N) as b:
        for ctx in (a, b):
            begin(M, rom, ctx, p, S)
        a.thermal_schedule(T_lo, T_hi, **tabs)
        A = collect(a, [a.step(m, outputs=KEYS, obs=("negSOC",), thermal=th, pack=("ucmd",)) for m in (7, 1, 32)])
        parts = []
        for _ in range(steps):
            T = b.thermal_get("T")["T"]
            b.set_limits(**{k: sched_eval(T, T_lo, T_hi, t) for k, t in tabs.items()})
            parts.append(b.step(1, outputs=KEYS, obs=("negSOC",), thermal=th, pack=("ucmd",)))
        B = collect(b, parts)
        la, lb = a.get_limits(), b.get_limits()
    compare(A, B, "schedule")
    for k in tabs:
        sr.bits_equal(la[k], lb[k], f"schedule: get_limits {k}")
    assert not np.array_equal(A["u"][:steps], base["u"][:steps]), "the schedule binds"
    assert (A["cond"] != 0).any()


# ---- 5. identity -------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["S1", "all_inf", "after_end"])
def test_identity(M, rom, base, how):
    series = 1 if how == "S1" else S
    p = dict(base["p"])
    if how == "all_inf":
        p["links"] = np.full(N, np.inf)
    calls = (1, 5, 24)
    plain = run_coupled(M, rom, N, series, calls, p=p, links=False)
    rows = tuple(k for k in ROWS if k != "cond")
    if how == "after_end":
        with M.Context(rom, N) as ctx:
            begin(M, rom, ctx, p, series)
            ctx.thermal_couple_end()
            with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_couple_get"):
                ctx.thermal_couple_get()
            with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_couple"):
                ctx.step(1, thermal="cond")
            got = collect(ctx, [ctx.step(m, outputs=KEYS, obs=("negSOC",), thermal=("temp", "heat"), pack=("ucmd",))
                                for m in calls], coupled=False)
            ctx.thermal_couple_end()                       # a no-op without links
    else:
        got = run_coupled(M, rom, N, series, calls, p=p)
        assert (got["cond"] == 0).all() and not np.signbit(got["cond"]).any()
        assert (got["crec"]["NB_SUM"] == 0).all() and np.isnan(got["crec"]["DT_MAX"]).all()
        assert (got["crec"]["DT_MAX_STEP"] == 0).all()
    compare(got, plain, how, rows=rows)
    assert not np.array_equal(plain["temp"][1:], base["temp"][1:30]) or series == 1


# ---- 6. the seed: T changed between two fused calls --------------------------------------------
def test_temperature_changed_between_calls(M, rom, base):
    p = base["p"]
    rng = np.random.Generator(np.random.PCG64(11))
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p, S)
        ctx.step(3, outputs=())
        for how in ("stage", "init", "begin"):
            Tn = rng.permutation(p["T0"]) + 1.5
            if how == "stage":
                ctx.OB_step(ctx.get_scalars(("uk",))["uk"], Tc=Tn)          # a stage call's temperature argument
            elif how == "init":
                ctx.init_cells(p["soc0"], Tn)
            else:
                ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom), T0=Tn)
            o = ctx.step(2, outputs=("u",), thermal=("temp", "cond"))
            sr.bits_equal(o["temp"][0], Tn, f"{how}: temp[0]")
            same(o["cond"][0], cr.conduct(Tn, p["links"], S)[0], f"{how}: cond[0] from the new temperatures")
            same(o["cond"][1], cr.conduct(o["temp"][1], p["links"], S)[0], f"{how}: cond[1]")
            assert (o["cond"][0] != cr.conduct(p["T0"], p["links"], S)[0]).any()
        r = ctx.thermal_couple_get()                                        # the second begin reset the record
        assert (ctx.thermal_get("steps")["steps"] == 2).all() and (r["DT_MAX_STEP"] <= 2).all()


# ---- 7. a cell in error ------------------------------------------------------------------------
def test_error_cell_still_conducts(M, rom, base):
    bad = 137                                  # string 10, position 7: a finite link on both sides
    p = base["p"]
    assert np.isfinite(p["links"][[bad - 1, bad]]).all()
    status = np.zeros(N, dtype=np.int32)
    status[bad] = ST_ERROR
    g = run_coupled(M, rom, N, S, (STEPS,), p=p, status=status)
    temp, heat, cond, th, cp = check_restated(rom, g, "error cell", status)
    assert th["nheld"][bad] == STEPS and (temp[:, bad] == p["T0"][bad]).all() and np.isnan(heat[:, bad]).all()
    assert np.isfinite(cond[:, bad]).all() and (cond[:, bad] != 0).all()
    assert (cond[:, [bad - 1, bad + 1]] != 0).all() and (temp[-1, [bad - 1, bad + 1]] != base["temp"][-1, [bad - 1, bad + 1]]).all()
    assert cp["NB_SUM"][bad] != 0 and cp["DT_MAX"][bad] > 0


# ---- 8. S = 2: the flows over a link cancel ----------------------------------------------------
def test_pair_flows_cancel(M, rom):
    g = run_coupled(M, rom, N, 2, (STEPS,))
    a, b = g["cond"][:, 0::2], g["cond"][:, 1::2]
    fin = np.isfinite(a) & np.isfinite(b)
    assert fin.all() and (a[fin] == -b[fin]).all()
    linked = np.isfinite(g["p"]["links"][0::2])
    assert (a[:, linked] != 0).all() and (a[:, ~linked] == 0).all() and (~linked).any()
    sr.bits_equal(g["crec"]["NB_SUM"][0::2], -g["crec"]["NB_SUM"][1::2] + 0.0, "NB_SUM")


# ---- 9. refusals change nothing ----------------------------------------------------------------
def test_refusals_change_nothing(M, rom):
    n, series = 12, 4
    p = params(n)
    ocv = M.thermal_ocv(rom)
    dp = C.POINTER(C.c_double)
    with M.Context(rom, n) as ctx, M.Context(rom, n) as twin:
        ctx.init_cells(p["soc0"], p["T0"])
        L, h = ctx.L, ctx.h
        link = np.ascontiguousarray(p["links"])
        call = lambda a: L.mpcekf_thermal_couple(h, None if a is None else a.ctypes.data_as(dp))
        assert call(link) == -5 and b"mpcekf_thermal_begin first" in L.mpcekf_last_error()
        ctx.pack_begin(series)
        assert call(link) == -5 and b"mpcekf_thermal_begin first" in L.mpcekf_last_error()
        ctx.pack_end()
        ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], ocv)
        assert call(link) == -5 and b"mpcekf_pack_begin first" in L.mpcekf_last_error()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_couple"):
            ctx.step(1, thermal="cond")
        ctx.pack_begin(series)
        begin(M, rom, twin, p, series)
        ctx.thermal_couple(p["links"])
        a, b = ctx.step(5, outputs=KEYS, thermal=("temp", "cond")), twin.step(5, outputs=KEYS, thermal=("temp", "cond"))
        st0, rec0, th0 = ctx.get_state(), ctx.thermal_couple_get(), ctx.thermal_get()

        def put(c, v):
            r = link.copy()
            r[c] = v
            return r
        assert call(None) == -1 and b"null r_link" in L.mpcekf_last_error()
        for c, v, msg in ((2, np.nan, b"r_link[2] = nan"), (0, 0.0, b"r_link[0] = 0"), (5, -1.5, b"r_link[5] = -1.5"),
                          (3, -np.inf, b"r_link[3] = -inf"), (n - 1, -2.0, b"r_link[11] = -2"),     # a string's last entry too
                          (series - 1, np.nan, b"r_link[3] = nan")):
            assert call(put(c, v)) == -1, (c, v)
            assert msg in L.mpcekf_last_error(), (msg, L.mpcekf_last_error())
        state_equal(ctx.get_state(), st0, "refused links")
        for k in CFIELDS:
            same(ctx.thermal_couple_get()[k], rec0[k], f"refused links: record {k}")
        for k in FIELDS:
            sr.bits_equal(ctx.thermal_get()[k], th0[k], f"refused links: thermal record {k}")
        a, b = ctx.step(5, outputs=KEYS, thermal=("temp", "cond")), twin.step(5, outputs=KEYS, thermal=("temp", "cond"))
        for k in a:                                 # the links in force are still the first ones
            same(a[k].astype(np.float64), b[k].astype(np.float64), f"after refused links: {k}")
        # a second set replaces the links and resets the record; pack_begin keeps the coupling
        ctx.thermal_couple(put(1, np.inf))
        r = ctx.thermal_couple_get()
        assert (r["NB_SUM"] == 0).all() and np.isnan(r["DT_MAX"]).all() and (r["DT_MAX_STEP"] == 0).all()
        T = ctx.thermal_get("T")["T"].copy()
        o = ctx.step(1, outputs=(), thermal="cond")
        same(o["cond"][0], cr.conduct(T, put(1, np.inf), series)[0], "replaced links")
        ctx.pack_begin(6)                           # the links follow the new strings
        T = ctx.thermal_get("T")["T"].copy()
        o = ctx.step(1, outputs=(), thermal="cond")
        same(o["cond"][0], cr.conduct(T, put(1, np.inf), 6)[0], "links after a second pack_begin")
        assert (ctx.thermal_couple_get()["DT_MAX_STEP"] > 0).any()
        ctx.pack_end()                              # ends the coupling implicitly
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_couple_get"):
            ctx.thermal_couple_get()
        ctx.pack_begin(series)
        ctx.thermal_couple(p["links"])
        ctx.thermal_end()                           # so does thermal_end
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_couple_get"):
            ctx.thermal_couple_get()


def test_wrappers_pass_the_links_through(M, rom, base):
    p = base["p"]
    th = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom), couple=p["links"])
    out = M.runMPC(rom, p["soc0"], p["T0"], 20, thermal=th, pack=dict(series=S))
    for k in KEYS + ("temp", "heat", "cond", "ucmd"):
        same(out[k].astype(np.float64), base[k][:20].astype(np.float64), f"runMPC: {k}")
    assert tuple(out["couple"]) == CFIELDS
    s = M.run_summary(rom, p["soc0"], p["T0"], STEPS, thermal=th, pack=dict(series=S), chunk=33)
    for k in CFIELDS:
        same(s["couple"][k], base["crec"][k], f"run_summary: coupling record {k}")
    for k in FIELDS:
        sr.bits_equal(s["thermal"][k], base["rec"][k], f"run_summary: thermal record {k}")
