"""GPU: side-reaction losses per cell along the fused loop (mpcekf_aging_begin / _get / _end,
mpcekf_step_ex_aging; k_aging once per fused step, before k_thermal).

What is compared with what: the reference is a second context WITHOUT aging, set up the same way
and stepped with step(n, obs=("negPhise0",), thermal=("temp",)) (without a thermal model the
temperature rows are the tc that was passed, or the initial temperature).  Its phise, negPhise0
and temperature rows go through tests/aging_ref.py, the numpy restatement of include/mpcekf.h's
rule (checked on the CPU in test_aging_ref.py).  The aging context's record, its rate rows and
every trajectory are compared with that, bit for bit (a NaN equals a NaN).  Nothing expected comes
from the code under test.

Shapes: 3, 257 and 1,000 cells (a partial block, two blocks, four blocks) and 110 steps (across
the 64-step window and flush); the routes 96 to 192 cells and 20 to 30 steps.
"""
import contextlib
import os
from importlib import import_module

import numpy as np
import pytest

import aging_ref as ar
import limit_groups as lg
from conftest import batch_inputs

pytestmark = pytest.mark.gpu

STEPS = 110
KEYS = ("u", "v", "soc", "phise", "nexec")
SRC = {"est": ("est",), "plant": ("plant",), "both": ("est", "plant")}
ST_ERROR = 1


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@contextlib.contextmanager
def _env(**env):
    """The host switches are read at context creation."""
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


def same(a, b, what=""):
    """Equal bits, or NaN on both sides; integers equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
    if not eq.all():
        i = tuple(np.argwhere(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {a.size} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def state_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        same(a[k], b[k], f"{what}: state {k}")


def reactions(n, nreact, gate=0.12, seed=0xA61):
    """Up to four reactions: plating gated at `gate` V, plating always on with an activation
    energy, one with per-cell i0 / alpha / Ea / gate arrays, an SEI-like one at U = 0.4 V."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = [dict(i0=1e-3, U=0.0, alpha=0.5, Ea=0.0, gate=gate),
            dict(i0=2e-4, U=0.0, alpha=0.5, Ea=3.0e4),
            dict(i0=rng.uniform(1e-4, 1e-3, n), U=0.0, alpha=rng.uniform(0.3, 0.7, n), Ea=rng.uniform(1e4, 6e4, n),
                 gate=rng.uniform(0.10, 0.16, n)),
            dict(i0=1e-6, U=0.4, alpha=0.3, Ea=5.0e4)]
    return pool[:nreact]


def setup(ctx, c):
    ctx.init_cells(c["soc0"], c["T0"])
    if c.get("status") is not None:
        st = ctx.get_state()
        st["status"] = c["status"]
        ctx.set_state(st)
    if c.get("limits"):
        ctx.set_limits(**c["limits"])
    if c.get("thermal"):
        ctx.thermal_begin(**c["thermal"])
    if c.get("schedule"):
        ctx.thermal_schedule(*c["schedule"][0], **c["schedule"][1])
    if c.get("pack"):
        ctx.pack_begin(c["pack"])
    ctx.set_graph(bool(c.get("graph")))


def case(n, steps=STEPS, **kw):
    soc0, T0 = batch_inputs(n)
    return dict(dict(n=n, steps=steps, soc0=soc0, T0=T0), **kw)


def reference(M, rom, c):
    """The context without aging: trajectories, the plant's negPhise0, the temperature each step
    used, the final state."""
    n, steps = c["n"], c["steps"]
    with _env(**c.get("env", {})), M.Context(rom, n, c.get("cfg")) as ctx:
        setup(ctx, c)
        out = ctx.step(steps, outputs=KEYS, tc=c.get("tc"), obs=("negPhise0",), thermal=("temp",) if c.get("thermal") else None)
        out["state"] = ctx.get_state()
        if c.get("thermal"):
            out["thermal"] = ctx.thermal_get()
    if not c.get("thermal"):
        out["temp"] = M.tc_grid(c["tc"], steps, n) if c.get("tc") is not None else np.broadcast_to(c["T0"], (steps, n))
    out["plant"] = out["obs"]["negPhise0"]
    return out


def expected(rom, ref, par, sources, t0=0, t1=None, recs=None):
    """aging_ref over the reference rows: {source: record}, rate [steps][nsrc * nreact][n]."""
    recs, rates = dict(recs or {}), []
    for s in sources:
        rows = ref["phise"] if s == "est" else ref["plant"]
        recs[s], rate = ar.run(rows[t0:t1], ref["temp"][t0:t1], par, float(rom.F), float(rom.R), float(rom.Tref), recs.get(s))
        rates.append(rate)
    return recs, np.concatenate(rates, axis=1)


def aging_run(M, rom, c, reacts, sources, calls=None, obs=None, summary=False, rate=True):
    """The aging context over the calls' steps: trajectories, rate rows, the record, the state."""
    n, steps = c["n"], c["steps"]
    calls = calls or (steps,)
    assert sum(calls) == steps
    tcs = None if c.get("tc") is None else M.tc_grid(c["tc"], steps, n)
    with _env(**c.get("env", {})), M.Context(rom, n, c.get("cfg")) as ctx:
        setup(ctx, c)
        ctx.aging_begin(reacts, sources=sources)
        parts, k = [], 0
        if summary:
            ctx.summary_begin(obs=obs)
        for m in calls:
            tc = None if tcs is None else tcs[k:k + m]
            if summary:
                ctx.step_summary(m, tc=tc)
            else:
                parts.append(ctx.step(m, outputs=KEYS, tc=tc, obs=obs, thermal=("temp",) if c.get("thermal") else None,
                                      aging=("rate",) if rate else None))
            k += m
        out = {}
        if parts:
            out = {q: np.concatenate([p[q] for p in parts]) for q in parts[0] if q != "obs"}
            if obs:
                out["obs"] = {q: np.concatenate([p["obs"][q] for p in parts]) for q in parts[0]["obs"]}
        if summary:
            out["summary"] = ctx.get_summary()
        out["rec"] = ctx.aging_record()
        out["state"] = ctx.get_state()
        if c.get("thermal"):
            out["thermal"] = ctx.thermal_get()
    return out


def compare(rom, got, ref, reacts, sources, what, traj=True):
    n = ref["phise"].shape[1]
    par = ar.params(n, reacts)
    recs, rate = expected(rom, ref, par, sources)
    assert set(got["rec"]) == set(sources)
    for s in sources:
        for r in range(len(reacts)):
            for k in ar.FIELDS:
                want = recs[s][k] if k in ("steps", "nskip") else recs[s][k][r]
                same(got["rec"][s][r][k], want, f"{what}: {s} reaction {r} {k}")
    if "rate" in got:
        same(got["rate"], rate, f"{what}: rate")
    if traj:
        for k in KEYS + (("temp",) if "thermal" in got else ()):
            same(got[k], ref[k], f"{what}: {k}")
    state_equal(got["state"], ref["state"], what)
    if "thermal" in got:
        for k in ref["thermal"]:
            same(got["thermal"][k], ref["thermal"][k], f"{what}: thermal record {k}")
    return recs, rate


def gated_share(rec, r=0):
    """The share of cells whose gated reaction was on for some steps and off for others."""
    return float(((rec["n_on"][r] > 0) & (rec["n_on"][r] < rec["steps"])).mean())


_REFS = {}


def base_ref(M, rom, n):
    """The default route's reference at n cells x 110 steps (shared, read-only)."""
    if n not in _REFS:
        c = case(n)
        ref = reference(M, rom, c)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[n] = (c, ref)
    return _REFS[n]


def plant_gate(rom, ref):
    """0.12 V where the plant's rows cross it in three quarters of the cells; else each cell's own
    median over its reference row (the gate is a per-cell parameter): a cell whose negPhise0 moves
    at all is then below its gate for some steps and not for others."""
    n = ref["plant"].shape[1]
    par = ar.params(n, [dict(i0=1e-3, U=0.0, alpha=0.5, Ea=0.0, gate=0.12)])
    rec, _ = ar.run(ref["plant"], ref["temp"], par, float(rom.F), float(rom.R), float(rom.Tref))
    return 0.12 if gated_share(rec) >= 0.75 else np.nanmedian(ref["plant"], axis=0)


# ---- 1. sizes, reaction counts, sources ---------------------------------------------------------
SIZES = [(257, nr, s) for nr in (1, 2, 4) for s in ("est", "plant", "both")] + \
        [(3, 1, "est"), (3, 2, "plant"), (3, 4, "both"), (1000, 4, "est"), (1000, 1, "plant"), (1000, 2, "both")]


@pytest.mark.parametrize("n,nreact,src", SIZES)
def test_sizes_reactions_sources(M, rom, n, nreact, src):
    c, ref = base_ref(M, rom, n)
    sources = SRC[src]
    # the precondition, on the reference rows alone: the gated reaction switches within the run
    gate = plant_gate(rom, ref) if src == "plant" else 0.12
    reacts = reactions(n, nreact, gate)
    recs, _ = expected(rom, ref, ar.params(n, reacts), sources)
    share = gated_share(recs[sources[0]])
    print(f"n = {n}, {src}: gate {np.mean(gate):.4f} V (mean), 0 < N_ON < STEPS in {share:.3f} of the cells; "
          f"plant - est: {np.nanmin(ref['plant'] - ref['phise']):+.4f} .. {np.nanmax(ref['plant'] - ref['phise']):+.4f} V")
    assert share >= 0.75
    if src == "both":
        # under "both" the two sources share the reactions, hence est's 0.12 V gate: only the est source is
        # asked to meet the cap there.  The plant's negPhise0 runs up to 0.035 V above the estimate and
        # crosses 0.12 V in fewer cells; the plant-only cases, with each cell's own median as its gate, meet
        # the cap for the plant source.  Its share here is printed, not asserted.
        print(f"n = {n}, both: the plant source at 0.12 V: 0 < N_ON < STEPS in {gated_share(recs['plant']):.3f} of the cells")
    assert (recs[sources[0]]["steps"] == STEPS).all()
    got = aging_run(M, rom, c, reacts, sources)
    _, rate = compare(rom, got, ref, reacts, sources, f"{n} cells, {nreact} reactions, {src}")
    assert rate.shape == (STEPS, len(sources) * nreact, n) and (rate > 0).any() and (rate == 0).any()
    if src == "both":   # the comparison the feature exists for: the EKF's phise error is visible
        assert not np.array_equal(got["rec"]["est"][0]["q_sum"], got["rec"]["plant"][0]["q_sum"])


# ---- 2. the temperature is the step's, not the advanced one ------------------------------------
def thermal_case(M, rom, n, steps, schedule=None, **kw):
    import test_gpu_thermal as tg
    p = tg.params(n)
    rng = np.random.Generator(np.random.PCG64(0x7AC6))
    c = case(n, steps, thermal=dict(Cth=rng.uniform(20.0, 60.0, n), Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom)),
             schedule=schedule, **kw)
    c["soc0"], c["T0"] = rng.uniform(10.0, 60.0, n), p["T0"]
    return c


def test_thermal_model_warms_the_cells(M, rom):
    n, steps = 257, 70
    c = thermal_case(M, rom, n, steps)
    ref = reference(M, rom, c)
    assert ((ref["temp"][-1] - ref["temp"][0]) > 1.0).mean() >= 0.25      # kelvins within the run
    reacts = reactions(n, 4)[1:]                                          # Ea != 0, per-cell arrays among them
    got = aging_run(M, rom, c, reacts, ("est", "plant"))
    recs, _ = compare(rom, got, ref, reacts, ("est", "plant"), "thermal")
    # the advanced temperature would have given other sums
    shifted = dict(ref, temp=np.concatenate([ref["temp"][1:], ref["thermal"]["T"][None]]))
    other, _ = expected(rom, shifted, ar.params(n, reacts), ("est",))
    assert (other["est"]["q_sum"][0] != recs["est"]["q_sum"][0]).mean() >= 0.25


# ---- 3. routes ---------------------------------------------------------------------------------
ROUTES = {
    # name: (n, steps, make_config keywords, per-cell limits?, environment, calls, graph)
    "mb": (192, 30, dict(method="MB"), False, {}, None, False),
    "mask_eta_off": (192, 30, dict(constraints=(1, 1, 0)), False, {}, None, False),
    "percell": (192, 30, {}, True, {}, None, False),
    "np20": (96, 20, dict(Np=20, Nc=10), False, {}, None, False),
    "ekf4": (192, 30, {}, False, dict(MPCEKF_QUAD=1), None, False),
    "split_cell": (192, 30, {}, False, dict(MPCEKF_QUAD=0, MPCEKF_SPLIT_CELL=1), None, False),
    "graph": (192, 30, {}, False, {}, (10, 10, 10), True),
    "n_calls_of_one": (192, 30, {}, False, {}, (1,) * 30, False),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(M, rom, route):
    n, steps, kw, percell, env, calls, graph = ROUTES[route]
    c = case(n, steps, cfg=M.make_config(**kw), limits=lg.limit_arrays(n) if percell else None, env=env, graph=graph)
    ref = reference(M, rom, dict(c, graph=False))
    reacts = reactions(n, 2, float(np.nanmedian(ref["phise"])))
    got = aging_run(M, rom, c, reacts, ("est", "plant"), calls=calls)
    recs, _ = compare(rom, got, ref, reacts, ("est", "plant"), route)
    assert (recs["est"]["n_on"][0] > 0).any() and (recs["est"]["n_on"][0] < steps).any()


def test_graph_replay_without_rows(M, rom):
    """One-step calls on a graph context with no output at all: the replayed graph reads the
    context's own phise and negPhise0 rows, and tt comes from the record."""
    n, steps = 192, 12
    c = case(n, steps, graph=True)
    ref = reference(M, rom, dict(c, graph=False))
    reacts = reactions(n, 2, float(np.nanmedian(ref["phise"])))
    with M.Context(rom, n) as ctx:
        setup(ctx, c)
        ctx.aging_begin(reacts, sources=("est", "plant"))
        for _ in range(steps):
            ctx.step(1, outputs=())
        got = dict(rec=ctx.aging_record(), state=ctx.get_state())
    recs, _ = compare(rom, got, ref, reacts, ("est", "plant"), "graph, no rows", traj=False)
    assert (recs["est"]["j_max_step"][0] > 1).any()


# ---- 4. step_summary, a pack, a schedule, a passed tc row ---------------------------------------
@pytest.mark.parametrize("slot", [None, "negPhise0", "cellSOC"])
def test_step_summary(M, rom, slot):
    n = 257
    c, ref = base_ref(M, rom, n)
    reacts = reactions(n, 2)
    got = aging_run(M, rom, c, reacts, ("est", "plant"), calls=(70, 40), obs=slot, summary=True)
    compare(rom, got, ref, reacts, ("est", "plant"), f"summary, slot {slot}", traj=False)
    same(got["summary"]["phise_min"], np.nanmin(ref["phise"], axis=0), "the summary itself")
    if slot == "negPhise0":
        same(got["summary"]["obs_min"], np.nanmin(ref["plant"], axis=0), "the summary's obs slot")


def test_pack_of_four(M, rom):
    n, steps = 192, 30
    c = case(n, steps, pack=4)
    c["soc0"] = np.linspace(10.0, 92.0, n)[np.random.Generator(np.random.PCG64(5)).permutation(n)]
    ref = reference(M, rom, c)
    free = reference(M, rom, dict(c, pack=None))
    assert (ref["u"] != free["u"]).mean() > 0.05                 # the strings couple something
    reacts = reactions(n, 2, float(np.nanmedian(ref["phise"])))
    got = aging_run(M, rom, c, reacts, ("est", "plant"))
    compare(rom, got, ref, reacts, ("est", "plant"), "pack")


def test_thermal_schedule(M, rom):
    n, steps = 192, 40
    grid = np.linspace(0.0, 1.0, 5)
    sched = ((20.0, 40.0), dict(sets=(np.arange(n) % 3).astype(np.int32),
                                Crate=np.stack([2.0 - 0.8 * grid, 1.6 - 0.5 * grid, 1.2 - 0.3 * grid])))
    c = thermal_case(M, rom, n, steps, schedule=sched)
    ref = reference(M, rom, c)
    reacts = reactions(n, 4)
    got = aging_run(M, rom, c, reacts, ("est", "plant"), calls=(25, 15))
    compare(rom, got, ref, reacts, ("est", "plant"), "schedule")


def test_passed_tc_rows(M, rom):
    n, steps = 192, 30
    rng = np.random.Generator(np.random.PCG64(0x7C))
    c = case(n, steps, tc=rng.uniform(18.0, 33.0, (steps, n)))
    ref = reference(M, rom, c)
    reacts = reactions(n, 4)[1:]                                 # Ea != 0: the passed row is the T of the rule
    got = aging_run(M, rom, c, reacts, ("est", "plant"), calls=(20, 10))
    recs, _ = compare(rom, got, ref, reacts, ("est", "plant"), "tc rows")
    held, _ = expected(rom, dict(ref, temp=np.broadcast_to(c["T0"], (steps, n))), ar.params(n, reacts), ("est",))
    assert (held["est"]["q_sum"][0] != recs["est"]["q_sum"][0]).mean() >= 0.75


# ---- 5. cells in error, end, a second begin, the caller's rows, refusals ------------------------
def test_error_cells_are_skipped(M, rom):
    n, steps = 70, 12
    status = np.zeros(n, dtype=np.int32)
    status[[0, 5, 64, 69]] = ST_ERROR
    c = case(n, steps, status=status)
    ref = reference(M, rom, c)
    assert np.isnan(ref["phise"][:, status != 0]).all() and np.isnan(ref["plant"][:, status != 0]).all()
    reacts = reactions(n, 2)
    got = aging_run(M, rom, c, reacts, ("est", "plant"))
    compare(rom, got, ref, reacts, ("est", "plant"), "error cells")
    for s in ("est", "plant"):
        rec = got["rec"][s][1]
        assert (rec["nskip"][status != 0] == steps).all() and (rec["steps"][status != 0] == 0).all()
        assert (rec["q_sum"][status != 0] == 0).all() and np.isnan(rec["j_max"][status != 0]).all()
        assert (rec["nskip"][status == 0] == 0).all() and (rec["q_sum"][status == 0] > 0).all()
    assert np.isnan(got["rate"][:, :, status != 0]).all() and not np.isnan(got["rate"][:, :, status == 0]).any()


def test_end_second_begin_and_callers_rows(M, rom):
    n = 70
    c = case(n, 30)
    ref = reference(M, rom, c)
    reacts = reactions(n, 2, float(np.nanmedian(ref["phise"])))
    par = ar.params(n, reacts)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for x in (a, b):
            setup(x, c)
        a.aging_end()                                              # a no-op without a begin
        a.aging_begin(reacts, sources=("est", "plant"))
        # the caller's obs rows with a plant source: its own slots, with and without negPhise0
        g1 = a.step(10, outputs=KEYS, obs=("cellSOC", "negPhise0"), aging=("rate",))
        r1 = b.step(10, outputs=KEYS, obs=("cellSOC", "negPhise0"))
        for k in ("cellSOC", "negPhise0"):
            same(g1["obs"][k], r1["obs"][k], f"obs rows: {k}")
        recs, rate = expected(rom, ref, par, ("est", "plant"), 0, 10)
        same(g1["rate"], rate, "rate, negPhise0 among the caller's slots")
        g2 = a.step(10, outputs=("u",), obs=("cellSOC", "Vcell"))  # not among them: the context's own launch
        r2 = b.step(10, outputs=("u",), obs=("cellSOC", "Vcell"))
        for k in ("cellSOC", "Vcell"):
            same(g2["obs"][k], r2["obs"][k], f"obs rows: {k}")
        recs, _ = expected(rom, ref, par, ("est", "plant"), 10, 20, recs)
        for s in ("est", "plant"):
            for k in ar.FIELDS:
                same(a.aging_get(s, 1)[k], recs[s][k] if k in ("steps", "nskip") else recs[s][k][1], f"after 20: {s} {k}")
        # a second begin resets the record (and may change nreact and the sources)
        a.aging_begin(reacts[:1], sources="plant")
        z = a.aging_get("plant", 0)
        assert (z["q_sum"] == 0).all() and np.isnan(z["j_max"]).all() and (z["steps"] == 0).all()
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: aging_get: source = 1"):
            a.aging_get("est", 0)
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: aging_get: react = 1"):
            a.aging_get("plant", 1)
        a.aging_end()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: aging_get"):
            a.aging_get("plant", 0)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_aging"):
            a.step(1, aging=("rate",))
        state_equal(a.get_state(), b.get_state(), "refused calls change nothing")
        x, y = a.step(10, outputs=KEYS), b.step(10, outputs=KEYS)   # as a context that never began
        for k in KEYS:
            same(x[k], y[k], f"after the end: {k}")
            same(x[k], ref[k][20:], f"after the end, against the reference: {k}")
        state_equal(a.get_state(), b.get_state(), "after the end")


def test_refusals_leave_the_record(M, rom):
    n = 12
    c = case(n, 16)
    ref = reference(M, rom, c)
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    reacts = reactions(n, 2, float(np.nanmedian(ref["phise"][:8])))
    with M.Context(rom, n) as ctx:
        ctx.aging_begin(reacts, sources=("est", "plant"))           # before init_cells
        with pytest.raises(M.MpcekfError, match="mpcekf error -5"):
            ctx.step(1, aging=("rate",))
        setup(ctx, c)
        ctx.step(8, outputs=())
        before, st = ctx.aging_record(), ctx.get_state()
        assert (before["est"][0]["steps"] == 8).all()
        par = ar.params(n, reacts)
        L, h = ctx.L, ctx.h

        def bad(k, v, r=1):
            """Other parameters throughout (an upload before the refusal would show in the next sums), and
            one value no begin takes in the last cell of reaction r."""
            p = par.copy()
            p[:, 0] *= 2.0
            p[:, 1] += 0.01
            p[r, k, n - 1] = v
            return p
        calls = [(2, 1, None), (0, 1, par), (5, 1, par), (2, 0, par), (2, 4, par), (2, -1, par)]
        calls += [(2, 1, bad(0, v)) for v in (-1e-9, np.nan, np.inf)]
        calls += [(2, 1, bad(k, v)) for k in (1, 3) for v in (np.nan, np.inf, -np.inf)]
        calls += [(2, 1, bad(2, v)) for v in (0.0, -0.5, np.nan, np.inf)] + [(2, 1, bad(4, np.nan, 0))]
        for nreact, mask, p in calls:
            assert L.mpcekf_aging_begin(h, nreact, mask, None if p is None else lib.dptr(np.ascontiguousarray(p))) == -1, \
                (nreact, mask)
        # every refused begin changed nothing: the record and the state bit for bit ...
        now = ctx.aging_record()
        for src in ("est", "plant"):
            for r in range(2):
                for k in ar.FIELDS:
                    same(now[src][r][k], before[src][r][k], f"record after the refused begins: {src} {r} {k}")
        state_equal(ctx.get_state(), st, "state after the refused begins")
        # ... and the sums go on from there with the parameters of the begin that stood
        ctx.step(8, outputs=())
        compare(rom, dict(rec=ctx.aging_record(), state=ctx.get_state()), ref, reacts, ("est", "plant"),
                "8 + 8 steps around the refused begins", traj=False)
        assert L.mpcekf_aging_begin(h, 2, 1, lib.dptr(bad(4, -np.inf))) == 0     # a gate of -inf: never on, not refused
        ctx.aging_begin(reacts)
        ctx.step(8, outputs=())
        mid = ctx.aging_record()
        ids, vals = np.arange(6, dtype=np.int32), np.zeros((6, n))
        for args in ((1, 0, 0, lib.iptr(ids), lib.dptr(vals)), (1, 0, 7, lib.iptr(ids), lib.dptr(vals)),
                     (1, 0, 2, None, lib.dptr(vals)), (1, 0, 2, lib.iptr(ids), None), (2, 0, 2, lib.iptr(ids), lib.dptr(vals)),
                     (3, 0, 2, lib.iptr(ids), lib.dptr(vals)), (1, 2, 2, lib.iptr(ids), lib.dptr(vals)),
                     (1, -1, 2, lib.iptr(ids), lib.dptr(vals)), (1, 0, 2, lib.iptr(np.array([1, 1], dtype=np.int32)), lib.dptr(vals)),
                     (1, 0, 1, lib.iptr(np.array([6], dtype=np.int32)), lib.dptr(vals))):
            assert L.mpcekf_aging_get(h, *args) == -1, args[:3]
        assert L.mpcekf_step_ex_aging(h, -1, None, None, None, 0, None, None, None, None, None, None, 0) == -1
        assert L.mpcekf_step_ex_aging(h, 1, None, None, None, 1, None, None, None, None, None, None, 0) == -1   # null slots
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_aging: temp / heat"):
            ctx.step(1, aging=("rate",), thermal=("temp",))
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_aging: ucmd / limiter"):
            ctx.step(1, aging=("rate",), pack=("ucmd",))
        with pytest.raises(M.MpcekfError, match="mpcekf error -1"):
            ctx.step(1, aging=("rate",), tc=np.full(n, 500.0))
        after = ctx.aging_record()
        for r in range(2):
            for k in ar.FIELDS:
                same(after["est"][r][k], mid["est"][r][k], f"record after the refusals: {r} {k}")
        assert (after["est"][0]["steps"] == 8).all()


# ---- 6. the wrappers, and a context without aging -----------------------------------------------
def test_wrappers_pass_the_model_through(M, rom):
    n = 9
    c, ref = base_ref(M, rom, 257)
    reacts = [{k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in d.items()} for d in reactions(257, 4)]
    ag = dict(reactions=reacts, sources=("est", "plant"))
    out = M.runMPC(rom, c["soc0"][:n], c["T0"][:n], 40, aging=ag)
    sub = {k: ref[k][:40, :n] for k in KEYS + ("plant", "temp")}
    recs, rate = expected(rom, sub, ar.params(n, reacts), ("est", "plant"))
    same(out["rate"], rate, "runMPC: rate")
    for k in KEYS:
        same(out[k], sub[k], f"runMPC: {k}")
    s = M.run_summary(rom, c["soc0"][:n], c["T0"][:n], 40, aging=ag, chunk=15)
    for o, who in ((out, "runMPC"), (s, "run_summary")):
        for src in ("est", "plant"):
            for r in range(4):
                for k in ar.FIELDS:
                    want = recs[src][k] if k in ("steps", "nskip") else recs[src][k][r]
                    same(o["aging"][src][r][k], want, f"{who}: {src} {r} {k}")
    same(s["u_last"], out["u"][-1], "run_summary: u_last")


def test_default_context_untouched(M, rom, oc):
    soc0, tc = batch_inputs(64)
    out = M.runMPC(rom, soc0, tc, 20)
    ref = oc.run(rom, soc0, tc, 20, nthreads=4)
    assert "rate" not in out and "aging" not in out
    for k in KEYS:
        lg.bitwise(out[k], ref[k], k)
