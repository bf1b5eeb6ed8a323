"""GPU: MPC limits mapped over (SOC estimate, cell temperature) inside the fused loop
(mpcekf_limit_map / _get / _end, mpcekf_step_ex_map; k_map before a call's first step, then
k_thermal_map, k_map_step after k_thermal_couple, or k_map_step alone at the end of every step).

The reference is the loop the feature replaces, on a second context without a map: every step
evaluates include/mpcekf.h's rule in numpy (tests/limit_map_ref.py) at the soc row of the step
before and thermal_get's T, passes the values to set_limits and runs step(1).  The mapped context
must give its bits: u, v, soc, phise, nexec of every step, the lim rows, get_limits, get_state
and the map's record.  All comparisons are bitwise.

Inputs (inputs() below; main_b asserts the preconditions on the reference loop): 300 cells (a
second, partial 256-thread block), 65 (a wave boundary) and 3; 40 steps (Ts = 1 s: a cell at 1C
moves 1.1 % SOC); the quintic synthetic ROM.  Initial SOC 10..85 % spread evenly and shuffled.
SOC grid 0.2..0.8 with 121 nodes (0.5 % apart: a cell at 0.5C or more crosses a node; the cells
below 20 % and above 80 % clamp).  Temperature grid 25..40 degC with 4 nodes; T0 22..43 degC (both
clamps), Cth 15..60 J/K, so a charging cell warms several kelvin and some cross a 5 K node; Rth
finite on the even cells, +inf on the odd ones.  Three mapped fields (Crate falling with SOC and
temperature, phise_min rising towards the top of charge and in the cold, v_max lowered when hot),
two table sets, cell c on set perm[c] % 2.
"""
from importlib import import_module

import numpy as np
import pytest

import limit_map_ref as lm
from test_gpu_thermal_schedule import sched_eval

pytestmark = pytest.mark.gpu

N, STEPS = 300, 40
CALLS = (7, 1, 32)
KEYS = ("u", "v", "soc", "phise", "nexec")
Z_LO, Z_HI, NZ = 0.2, 0.8, 121
T_LO, T_HI, NT = 25.0, 40.0, 4
REC = ("z_last", "neval", "nclamp_z", "nclamp_t")


@pytest.fixture(scope="module")
def M(P):
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def inputs(n=N):
    rng = np.random.Generator(np.random.PCG64(0x11A9))
    soc0 = rng.permutation(np.linspace(10.0, 85.0, N))
    Rth = rng.uniform(2.0, 6.0, N)
    Rth[1::2] = np.inf
    p = dict(soc0=soc0, T0=rng.uniform(22.0, 43.0, N), Cth=rng.uniform(15.0, 60.0, N), Rth=Rth,
             Tamb=rng.uniform(15.0, 30.0, N), sets=(rng.permutation(N) % 2).astype(np.int32))
    return {k: np.ascontiguousarray(v[:n]) for k, v in p.items()}


def maps(nt=NT, nz=NZ, scale=1.0):
    """Two table sets [2][nt][nz] of three fields; no two neighbouring entries are equal."""
    z = np.linspace(0.0, 1.0, nz)[None, None, :] if nz > 1 else np.full((1, 1, 1), 0.5)
    t = np.linspace(0.0, 1.0, nt)[None, :, None] if nt > 1 else np.zeros((1, 1, 1))
    s = np.array([1.0, 0.9])[:, None, None]
    crate = scale * s * (2.0 - 1.3 * z ** 1.5) * (1.0 - 0.35 * t * t)
    phise = 0.08 + 0.03 * z * z * s + 0.02 * (1.0 - t) ** 2
    vmax = 4.1 - 0.08 * t ** 3 * s - 0.01 * z
    return dict(Crate=crate, phise_min=phise, v_max=vmax)


def same(a, b, what):
    """Equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if not eq.all():
        i = tuple(np.argwhere(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {a.size} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def state_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if a[k].dtype.kind == "f":
            same(a[k], b[k], f"{what}: state {k}")
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: state {k}"


def begin(M, rom, ctx, p, thermal=True, status=None, ext=()):
    """init_cells, the model and the extensions of a route, the same on both contexts."""
    n = p["soc0"].shape[0]
    ctx.init_cells(p["soc0"], p["T0"])
    if status is not None:
        st = ctx.get_state()
        st["status"] = status
        ctx.set_state(st)
    if thermal:
        ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))
    if "pack" in ext:
        ctx.pack_begin(4)
    if "balance" in ext:
        ctx.balance_begin(i_bleed=0.5, dz_on=0.02, dz_off=0.01)
    if "charger" in ext:
        ctx.charger_begin(i_max=50.0, p_max=700.0)
    if "couple" in ext:
        ctx.thermal_couple(np.where(np.arange(n) % 3 == 2, np.inf, 1.5))
    if "term" in ext:
        ctx.term_begin(soc_stop=0.78, i_taper=2.0, hold=3)


def collect(ctx, parts, thermal):
    out = {k: np.concatenate([q[k] for q in parts]) for k in KEYS + ("lim",)} if parts else {}
    out.update(limits=ctx.get_limits(), state=ctx.get_state())
    if thermal:
        out["thermal"] = ctx.thermal_get()
    return out


def map_args(p, tabs, thermal, sets, interp):
    kw = dict(sets=p["sets"] if sets else None, interp_z=interp, **tabs)
    if thermal and next(iter(tabs.values())).ndim >= 2 and next(iter(tabs.values())).shape[-2] > 1:
        kw.update(T_lo=T_LO, T_hi=T_HI)
    return kw


def run_mapped(M, rom, p, calls, tabs, cfg=None, thermal=True, sets=True, interp="linear", graph=False, status=None,
               ext=(), swap=None):
    """Context A: the map inside the fused calls.  swap = (call index, tables): the map replaced
    before that call."""
    with M.Context(rom, p["soc0"].shape[0], cfg) as ctx:
        begin(M, rom, ctx, p, thermal, status, ext)
        ctx.set_graph(graph)
        ctx.limit_map(Z_LO, Z_HI, **map_args(p, tabs, thermal, sets, interp))
        parts = []
        for i, m in enumerate(calls):
            if swap and swap[0] == i:
                ctx.limit_map(Z_LO, Z_HI, **map_args(p, swap[1], thermal, sets, interp))
            parts.append(ctx.step(m, outputs=KEYS, limit_map=("lim",)))
        out = collect(ctx, parts, thermal)
        out["rec"] = ctx.limit_map_get()
        return out


def run_host_driven(M, rom, p, nsteps, tabs, cfg=None, thermal=True, sets=True, interp="linear", status=None, ext=(),
                    swap=None):
    """Context B: no map; every step evaluates the rule in numpy, set_limits, step(1).  swap =
    (step index, tables): the tables replaced before that step (the record's counts restart)."""
    hold = int(interp == "hold")
    with M.Context(rom, p["soc0"].shape[0], cfg) as ctx:
        begin(M, rom, ctx, p, thermal, status, ext)
        rec = lm.Record(p["soc0"] / 100.0)
        parts, jz, jt = [], [], []
        for k in range(nsteps):
            if swap and swap[0] == k:
                tabs = swap[1]
                rec.neval[:], rec.nclamp_z[:], rec.nclamp_t[:] = 0.0, 0.0, 0.0
            T = ctx.thermal_get("T")["T"] if thermal else None
            jz.append(lm.axis(rec.z_last, Z_LO, Z_HI, NZ)[0])
            jt.append(lm.axis(T, T_LO, T_HI, NT)[0] if thermal else np.zeros_like(jz[-1]))
            vals = rec.evaluate(T, Z_LO, Z_HI, T_LO, T_HI, tabs, p["sets"] if sets else None, hold)
            ctx.set_limits(**vals)
            q = ctx.step(1, outputs=KEYS)
            q["lim"] = np.stack([vals[f] for f in tabs])[None]
            rec.store(q["soc"][0])
            parts.append(q)
        out = collect(ctx, parts, thermal)
        out.update(rec=rec.as_dict(), jz=np.stack(jz), jt=np.stack(jt))
        return out


def compare(a, b, what, fields):
    for k in KEYS + ("lim",):
        same(a[k], b[k], f"{what}: {k}")
    for k in a["limits"]:
        same(a["limits"][k], b["limits"][k], f"{what}: get_limits {k}")
    for k in REC:
        same(a["rec"][k], b["rec"][k], f"{what}: record {k}")
    if "thermal" in a:
        for k in a["thermal"]:
            same(a["thermal"][k], b["thermal"][k], f"{what}: thermal record {k}")
    state_same(a["state"], b["state"], what)
    for i, f in enumerate(fields):          # the values in force after the call are those its last step used
        same(a["limits"][f], a["lim"][-1, i], f"{what}: limits {f} are the last step's")


@pytest.fixture(scope="module")
def main_b(M, rom):
    """The reference loop of the main case (300 cells, a model, two sets, linear), with the
    preconditions that make a pass mean something."""
    p = inputs()
    b = run_host_driven(M, rom, p, STEPS, maps())
    assert ((b["jz"] != b["jz"][0]).any(axis=0)).mean() >= 0.25, "a quarter of the cells change jz"
    assert (b["jt"] != b["jt"][0]).any(), "a cell changes jt"
    assert (b["rec"]["nclamp_z"] > 0).any() and (b["rec"]["nclamp_t"] > 0).any(), "an evaluation clamps on each axis"
    assert (b["rec"]["nclamp_z"] == 0).any() and (b["rec"]["nclamp_t"] == 0).any()
    assert (b["rec"]["neval"] == STEPS).all()
    with M.Context(rom, N) as ctx:          # a map-free context computes something else
        begin(M, rom, ctx, p)
        assert (ctx.step(STEPS, outputs=("u",))["u"] != b["u"]).any(), "the map binds"
    assert np.isfinite(b["u"]).all() and (b["state"]["status"] == 0).all()
    return b


@pytest.fixture(scope="module")
def main_a(M, rom):
    return run_mapped(M, rom, inputs(), CALLS, maps())


# ---- 1. parity with the host-driven loop ------------------------------------------------------
def test_linear_map_with_a_model_and_two_sets(main_a, main_b):
    assert set(inputs()["sets"].tolist()) == {0, 1}
    compare(main_a, main_b, "linear", maps())
    same(main_a["lim"][0, 0], lm.map_eval(inputs()["soc0"] / 100.0, inputs()["T0"], Z_LO, Z_HI, T_LO, T_HI,
                                          maps()["Crate"], inputs()["sets"])[0], "lim[0] is the map at z0 and T0")


def test_one_step_calls_and_graph_replay_are_the_n_step_call(M, rom, main_a, main_b):
    compare(run_mapped(M, rom, inputs(), (1,) * STEPS, maps()), main_b, "one-step calls", maps())
    g = run_mapped(M, rom, inputs(), (10,) * 4, maps(), graph=True)
    compare(g, main_b, "graph replay", maps())


def test_map_with_fewer_fields_between_graph_replays(M, rom):
    """The lim rows' length is part of what a captured graph holds: a 3-field map replaced by a
    1-field one (and back) between calls of one shape must not replay the other stride."""
    p = inputs(65)
    one = dict(phise_min=maps()["phise_min"])
    with M.Context(rom, 65) as ctx:
        begin(M, rom, ctx, p)
        ctx.set_graph(True)
        parts, tabs_of = [], (maps(), maps(), one, one, maps(scale=0.8), maps(scale=0.8))
        for i, tabs in enumerate(tabs_of):
            if i % 2 == 0:
                ctx.limit_map(Z_LO, Z_HI, **map_args(p, tabs, True, True, "linear"))
            parts.append(ctx.step(5, outputs=KEYS, limit_map=("lim",)))
        state = ctx.get_state()
    with M.Context(rom, 65) as ctx:                # the reference loop, the tables switched at the same steps
        begin(M, rom, ctx, p)
        rec = lm.Record(p["soc0"] / 100.0)
        for i, tabs in enumerate(tabs_of):
            assert parts[i]["lim"].shape == (5, len(tabs), 65)
            for k in range(5):
                vals = rec.evaluate(ctx.thermal_get("T")["T"], Z_LO, Z_HI, T_LO, T_HI, tabs, p["sets"])
                if "Crate" not in vals:            # a dropped field goes back to the configuration's value
                    vals = dict(vals, Crate=np.full(65, 2.0), v_max=np.full(65, 4.1))
                ctx.set_limits(**vals)
                q = ctx.step(1, outputs=KEYS)
                rec.store(q["soc"][0])
                for j, f in enumerate(tabs):
                    same(parts[i]["lim"][k, j], vals[f], f"call {i} step {k}: lim {f}")
                for f in KEYS:
                    same(parts[i][f][k], q[f][0], f"call {i} step {k}: {f}")
        state_same(state, ctx.get_state(), "fewer fields between replays")


def test_map_replaced_between_graph_replays(M, rom):
    p, second = inputs(65), maps(scale=0.8)
    a = run_mapped(M, rom, p, (10,) * 4, maps(), graph=True, swap=(2, second))
    b = run_host_driven(M, rom, p, STEPS, maps(), swap=(20, second))
    assert (b["rec"]["neval"] == 20).all()
    compare(a, b, "replaced between replays", maps())


@pytest.mark.parametrize("arm", ["hold", "n3", "mb", "mask", "wide", "percell_despite_quad_env", "percell_despite_split_env"])
def test_routes(M, rom, monkeypatch, arm):
    """The last two arms are not k_ekf4 / split-k_cell coverage: a mapped context is on the per-cell
    launch sequence, which runs neither kernel (step_impl: quad && !lim, split_cell && !lim).  They
    check that a context asked for those routes by its environment still runs the per-cell
    sequence under a map, with the reference loop's bits."""
    kw = dict(mb=dict(method="MB"), mask=dict(constraints=(1, 1, 0)), wide=dict(Np=20, Nc=10)).get(arm, {})
    if arm == "percell_despite_quad_env":
        monkeypatch.setenv("MPCEKF_QUAD", "1")
    if arm == "percell_despite_split_env":
        monkeypatch.setenv("MPCEKF_SPLIT_CELL", "1")
    p = inputs(dict(n3=3, hold=N).get(arm, 65))
    interp = "hold" if arm == "hold" else "linear"
    cfg = M.make_config(**kw)
    a = run_mapped(M, rom, p, CALLS, maps(), cfg, interp=interp)
    b = run_host_driven(M, rom, p, STEPS, maps(), cfg, interp=interp)
    compare(a, b, arm, maps())


def test_no_temperature_axis_needs_no_model(M, rom):
    p = inputs(65)
    tabs = maps(nt=1)                                              # [2][1][nz]
    a = run_mapped(M, rom, p, CALLS, tabs, thermal=False)
    b = run_host_driven(M, rom, p, STEPS, tabs, thermal=False)
    compare(a, b, "nt == 1", tabs)
    assert (a["rec"]["nclamp_t"] == 0).all() and (a["rec"]["nclamp_z"] > 0).any()


@pytest.mark.parametrize("ext", [("pack", "balance", "charger"), ("pack", "couple"), ("term",)], ids=lambda e: "+".join(e))
def test_extensions(M, rom, ext):
    p = inputs(N if "pack" in ext else 65)
    a = run_mapped(M, rom, p, CALLS, maps(), ext=ext)
    b = run_host_driven(M, rom, p, STEPS, maps(), ext=ext)
    compare(a, b, "+".join(ext), maps())


def test_step_summary_and_step_until(M, rom, main_a):
    p = inputs()
    with M.Context(rom, N) as ctx:
        begin(M, rom, ctx, p)
        ctx.limit_map(Z_LO, Z_HI, **map_args(p, maps(), True, True, "linear"))
        ctx.summary_begin()
        for m in CALLS:
            ctx.step_summary(m)
        state_same(ctx.get_state(), main_a["state"], "step_summary")
        for k in REC:
            same(ctx.limit_map_get()[k], main_a["rec"][k], f"step_summary: record {k}")
        for k, v in ctx.get_limits().items():
            same(v, main_a["limits"][k], f"step_summary: limits {k}")
        same(ctx.get_summary("u_last")["u_last"], main_a["u"][-1], "step_summary: u_last")
    p = inputs(65)
    with M.Context(rom, 65) as ctx:
        begin(M, rom, ctx, p, ext=("term",))
        ctx.limit_map(Z_LO, Z_HI, **map_args(p, maps(), True, True, "linear"))
        run, open_cells = ctx.step_until(STEPS, chunk=16)
        b = run_host_driven(M, rom, p, run, maps(), ext=("term",))
        assert run == STEPS and 0 < open_cells < 65, "some cells latch, the loop runs its cap"
        state_same(ctx.get_state(), b["state"], "step_until")
        for k in REC:
            same(ctx.limit_map_get()[k], b["rec"][k], f"step_until: record {k}")
        for k, v in ctx.get_limits().items():
            same(v, b["limits"][k], f"step_until: limits {k}")


def test_error_cell_reads_the_first_column(M, rom):
    p = inputs(65)
    status = np.zeros(65, dtype=np.int32)
    status[[2, 64]] = 1                                            # MPCEKF_ST_ERROR: NaN outputs from the first step on
    a = run_mapped(M, rom, p, CALLS, maps(), status=status)
    b = run_host_driven(M, rom, p, STEPS, maps(), status=status)
    compare(a, b, "error cell", maps())
    assert np.isnan(a["soc"][:, [2, 64]]).all() and np.isnan(a["rec"]["z_last"][[2, 64]]).all()
    # the first evaluation is at z0; every later one at a NaN estimate, which clamps and is counted
    assert (a["rec"]["nclamp_z"][[2, 64]] >= STEPS - 1).all() and (a["rec"]["neval"] == STEPS).all()


# ---- 2. the two consequences of the rule -------------------------------------------------------
def test_nz_1_is_the_thermal_schedule(M, rom):
    p = inputs(65)
    tabs = maps(nz=1)                                              # [2][nt][1]
    a = run_mapped(M, rom, p, CALLS, tabs)
    with M.Context(rom, 65) as ctx:
        begin(M, rom, ctx, p)
        ctx.thermal_schedule(T_LO, T_HI, sets=p["sets"], **{k: v[:, :, 0] for k, v in tabs.items()})
        parts = [ctx.step(m, outputs=KEYS, thermal=("temp",)) for m in CALLS]
        # the schedule's values of every step, from the temperatures the steps used
        lim = lambda q: np.stack([np.stack([sched_eval(t, T_LO, T_HI, v[:, :, 0], p["sets"]) for v in tabs.values()])
                                  for t in q["temp"]])
        b = collect(ctx, [dict(q, lim=lim(q)) for q in parts], True)
    for k in KEYS + ("lim",):
        same(a[k], b[k], f"nz == 1: {k}")
    for k in a["limits"]:
        same(a["limits"][k], b["limits"][k], f"nz == 1: get_limits {k}")
    state_same(a["state"], b["state"], "nz == 1")
    assert (a["lim"][0] != a["lim"][-1]).any()


@pytest.mark.parametrize("thermal", [True, False], ids=["model", "no_model"])
def test_constant_tables_are_the_map_free_context(M, rom, thermal):
    p = inputs(65)
    cfg = M.make_config()
    shape = (2, NT, NZ) if thermal else (NZ,)
    tabs = dict(Crate=np.full(shape, cfg.Crate), phise_min=np.full(shape, cfg.phise_min))
    a = run_mapped(M, rom, p, CALLS, tabs, thermal=thermal, sets=thermal)
    with M.Context(rom, 65) as ctx:
        begin(M, rom, ctx, p, thermal)
        b = collect(ctx, [dict(ctx.step(m, outputs=KEYS), lim=np.empty((m, 2, 65))) for m in CALLS], thermal)
    for k in KEYS:
        same(a[k], b[k], f"constant tables: {k}")
    state_same(a["state"], b["state"], "constant tables")
    assert (a["lim"][:, 0] == cfg.Crate).all() and (a["lim"][:, 1] == cfg.phise_min).all()
    if thermal:
        for k in a["thermal"]:
            same(a["thermal"][k], b["thermal"][k], f"constant tables: thermal record {k}")


# ---- 3. coexistence and refusals ----------------------------------------------------------------
def test_replace_end_restores_and_the_schedule_is_excluded(M, rom):
    n = 65
    p = inputs(n)
    tabs = maps()
    crate, vmax = np.linspace(1.0, 1.9, n), np.linspace(4.0, 4.1, n)
    sched = {k: v[0, :, 0] for k, v in maps(nz=1).items()}
    with M.Context(rom, n) as ctx, M.Context(rom, n) as plain:
        for c in (ctx, plain):
            c.init_cells(p["soc0"], p["T0"])
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: limit_map: nt = 4: call mpcekf_thermal_begin first"):
            ctx.limit_map(Z_LO, Z_HI, T_lo=T_LO, T_hi=T_HI, Crate=tabs["Crate"])
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: limit_map_get: call mpcekf_limit_map first"):
            ctx.limit_map_get()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_map: call mpcekf_limit_map first"):
            ctx.step(1, limit_map=("lim",))
        ctx.limit_map_end()                                               # a no-op without a map
        for c in (ctx, plain):
            c.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))
            c.set_limits(Crate=crate, v_max=vmax)
        # argument refusals on a live context: nothing changes
        for kw, msg in ((dict(z_lo=0.5, z_hi=0.5), "SOC grid"), (dict(z_lo=0.0, z_hi=np.inf), "SOC grid"),
                        (dict(T_lo=40.0, T_hi=25.0), "temperature grid"), (dict(z0=np.inf), r"z0\[0\] = inf"),
                        (dict(sets=np.full(n, 2)), r"set_of_cell\[0\] = 2 outside 0..1"),
                        (dict(Crate=np.where(np.arange(NZ) == 7, np.nan, tabs["Crate"])), r"tables\[7\] = nan")):
            args = dict(dict(z_lo=Z_LO, z_hi=Z_HI, T_lo=T_LO, T_hi=T_HI, Crate=tabs["Crate"]), **kw)
            with pytest.raises(M.MpcekfError, match="mpcekf error -1: limit_map: .*" + msg):
                ctx.limit_map(**args)
        ids = np.array([1], dtype=np.int32)
        lib = import_module("mpc-ekf4fastcharge_amd._lib")
        for nz_, nt_, interp_, msg in ((1, 1, 0, b"nz = 1, nt = 1"), (0, 2, 0, b"nz = 0"), (1, 2, 2, b"interp_z = 2")):
            assert ctx.L.mpcekf_limit_map(ctx.h, 1, lib.iptr(ids), nz_, 0.0, 1.0, nt_, 20.0, 40.0, interp_, 1,
                                          lib.dptr(np.ones((1, 1, 2, 2))), None, None) == -1
            assert msg in ctx.L.mpcekf_last_error()
        # the refusals the wrapper would raise for first, straight at the library
        I, tab4 = lib.iptr, lib.dptr(np.ones((1, 6, 2, 2)))
        F = lambda *x: np.array(x, dtype=np.int32)
        for nf_, f_, t_, nsets_, msg in ((2, None, tab4, 1, b"null fields"), (2, I(F(1, 6)), None, 1, b"null tables"),
                                         (0, I(F(1)), tab4, 1, b"nfields = 0 outside 1..6"),
                                         (7, I(F(*range(7))), tab4, 1, b"nfields = 7 outside 1..6"),
                                         (2, I(F(1, 1)), tab4, 1, b"id 1 given twice"),
                                         (2, I(F(1, 0)), tab4, 1, b"fields[1] = 0 cannot be mapped"),
                                         (2, I(F(7, 1)), tab4, 1, b"fields[0] = 7 cannot be mapped"),
                                         (2, I(F(1, 9)), tab4, 1, b"fields[1] = 9 cannot be mapped"),
                                         (2, I(F(1, 6)), tab4, 0, b"nsets = 0"), (2, I(F(1, 6)), tab4, -1, b"nsets = -1")):
            assert ctx.L.mpcekf_limit_map(ctx.h, nf_, f_, 2, 0.0, 1.0, 2, 20.0, 40.0, 0, nsets_, t_, None, None) == -1, msg
            assert msg in ctx.L.mpcekf_last_error(), (msg, ctx.L.mpcekf_last_error())
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: limit_map_get"):   # none of them began a map
            ctx.limit_map_get()
        same(ctx.get_limits()["Crate"], crate, "after refusals")
        # a map of Crate and phise_min, then one of phise_min alone: Crate goes back to set_limits' array
        ctx.limit_map(Z_LO, Z_HI, T_lo=T_LO, T_hi=T_HI, sets=p["sets"], Crate=tabs["Crate"], phise_min=tabs["phise_min"])
        assert (ctx.get_limits()["Crate"] != crate).any()
        same(ctx.get_limits()["phise_min"], lm.map_eval(p["soc0"] / 100.0, p["T0"], Z_LO, Z_HI, T_LO, T_HI,
                                                        tabs["phise_min"], p["sets"])[0], "evaluated when set")
        assert (ctx.limit_map_get()["neval"] == 0).all()
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: set_limits: .* is mapped over SOC and temperature"):
            ctx.set_limits(v_max=4.0, Crate=1.0)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: clear_limits: a limit map is active"):
            ctx.clear_limits()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: thermal_schedule: a limit map is active"):
            ctx.thermal_schedule(T_LO, T_HI, **sched)
        same(ctx.get_limits()["v_max"], vmax, "v_max after refusals")
        ctx.step(5, outputs=())
        ctx.limit_map(Z_LO, Z_HI, T_lo=T_LO, T_hi=T_HI, sets=p["sets"], phise_min=tabs["phise_min"])
        same(ctx.get_limits()["Crate"], crate, "a dropped field goes back to set_limits' values")
        rec = ctx.limit_map_get()
        assert (rec["neval"] == 0).all() and np.isfinite(rec["z_last"]).all() and (rec["z_last"] != p["soc0"] / 100.0).any()
        ctx.limit_map_end()
        lim = ctx.get_limits()
        same(lim["Crate"], crate, "Crate after end")
        same(lim["v_max"], vmax, "v_max after end")
        assert (lim["phise_min"] == 0.08).all()
        # the context goes on as one that only ever had set_limits
        plain.set_state(ctx.get_state())
        plain.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom), T0=ctx.thermal_get("T")["T"])
        plain.set_limits(Crate=crate, v_max=vmax)
        a, b = (c.step(6, outputs=KEYS) for c in (ctx, plain))
        for k in KEYS:
            same(a[k], b[k], f"after limit_map_end: {k}")
        ctx.clear_limits()                                                # allowed again
        # the other order: a schedule first refuses the map; thermal_end ends a map with a temperature axis
        ctx.thermal_schedule(T_LO, T_HI, **sched)
        before = ctx.get_limits()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: limit_map: a temperature schedule is active"):
            ctx.limit_map(Z_LO, Z_HI, Crate=tabs["Crate"][0, 0])
        for k, v in ctx.get_limits().items():
            same(v, before[k], f"a refused map changes nothing: {k}")
        ctx.thermal_schedule_end()
        ctx.limit_map(Z_LO, Z_HI, T_lo=T_LO, T_hi=T_HI, Crate=tabs["Crate"])
        ctx.thermal_end()
        assert (ctx.get_limits()["Crate"] == 2.0).all()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: limit_map_get"):
            ctx.limit_map_get()
        # no temperature axis: no model needed.  The context has stepped since init_cells, so a NULL z0 is NaN
        ctx.limit_map(Z_LO, Z_HI, Crate=tabs["Crate"][0, 0])
        same(ctx.get_limits()["Crate"], np.full(n, tabs["Crate"][0, 0, 0]), "no z0 after steps: the first column")
        assert np.isnan(ctx.limit_map_get()["z_last"]).all()
        ctx.limit_map_end()
        ctx.limit_map(Z_LO, Z_HI, z0=a["soc"][-1], Crate=tabs["Crate"][0, 0])
        ctx.thermal_begin(p["Cth"], p["Rth"], p["Tamb"], M.thermal_ocv(rom))
        ctx.thermal_end()                                                 # and the model's end leaves it
        assert (ctx.limit_map_get()["neval"] == 0).all() and (ctx.get_limits()["Crate"] != 2.0).any()


def test_wrappers_pass_the_map_through(M, rom, main_a):
    p, n, steps = inputs(), 9, 8
    th = dict(Cth=p["Cth"][:n], Rth=p["Rth"][:n], Tamb=p["Tamb"][:n], ocv=M.thermal_ocv(rom))
    mp = dict(z_lo=Z_LO, z_hi=Z_HI, T_lo=T_LO, T_hi=T_HI, sets=p["sets"][:n], **maps())
    out = M.runMPC(rom, p["soc0"][:n], p["T0"][:n], steps, thermal=th, limit_map=mp)
    for k in ("u", "v", "soc", "lim"):
        same(out[k], main_a[k][:steps, ..., :n], f"runMPC: {k}")
    assert (out["limit_map"]["neval"] == steps).all()
    s = M.run_summary(rom, p["soc0"][:n], p["T0"][:n], steps, thermal=th, limit_map=mp, chunk=3)
    same(s["u_last"], out["u"][-1], "run_summary: u_last")
    same(s["limit_map"]["z_last"], out["soc"][-1], "run_summary: z_last")
