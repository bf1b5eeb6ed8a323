"""GPU: series strings along the fused loop (mpcekf_pack_begin / _get / _end, mpcekf_step_ex_pack;
k_pack after Hildreth in every fused step).

The reference everywhere is the host-driven loop the feature replaces, on a second context that
has no pack: per step, step(1), get_state, tests/pack_ref.py (the header's rule in plain Python)
on the uk column, uk / uk_1 written back with set_state({"scal": ...}).  Every comparison is
bitwise (a NaN equals a NaN).  Nothing expected comes from the code under test.

  1. precondition: the loop's get_state / set_state round trip perturbs nothing on a plain context
  2. host loop == fused pack over S in {2, 3, 5, 64, 96, 100, 256, 257, 1000}
  3. S = 1 is the identity
  4. ties and NaN cells by construction
  5. routes (MB, a mask, Np = 20, k_ekf4, the split k_cell, graph replay, call splitting, end)
  6. with the thermal model and a schedule
  7. with step_summary
  8. refusals
"""
import contextlib
import os

import numpy as np
import pytest

import pack_ref as pr
import summary_ref as sr

pytestmark = pytest.mark.gpu

KEYS = ("u", "v", "soc", "phise", "nexec")
S_UK_1, S_UK = 5, 6          # MPCEKF_S_UK_1, MPCEKF_S_UK
NSTEPS = 40
# S -> strings: two blocks or more for the strings that share a block (floor(256 / S) per block),
# strings across a wave boundary wherever 64 % S != 0, 2 to 3 blocks for the long ones
SHAPES = {2: 200, 3: 120, 5: 70, 64: 6, 96: 5, 100: 5, 256: 3, 257: 3, 1000: 2}


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


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


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


def inputs(n, S, seed=0x9ACC):
    """An SOC0 spread of 10..60 %, per-cell Crate among 1, 1.5, 2 (the string's first cell 1: the
    limiter while every cell sits on its current bound) and, last in every string, two cells
    (one at S = 2) at 70..90 % with Crate 2: near the 95 % target their voltage limit binds and
    their commands taper through the 1 C bound during the run, each at its own pace.  A per-cell
    target_soc a fraction of a percent ahead was tried first and tapers nothing within 60 steps.
    The reference loop under these inputs, 40 steps: at every S of SHAPES at least one string
    changes its limiter (1 of 3 at S = 256 / 257, 122 of 200 at S = 2) and ucmd != u in 0.50
    (S = 2) to 0.98 of the (cell, step) pairs."""
    rng = np.random.Generator(np.random.PCG64(seed + S))
    idx = np.arange(n) % S
    soc0 = rng.uniform(10.0, 60.0, n)
    crate = rng.choice(np.array([1.0, 1.5, 2.0]), n)
    crate[idx == 0] = 1.0
    for j in range(min(2, S - 1)):
        high = idx == S - 1 - j
        soc0[high] = rng.uniform(70.0, 90.0, int(high.sum()))
        crate[high] = 2.0
    return soc0, np.full(n, 25.0), dict(Crate=crate)


def setup(ctx, soc0, tc, limits=None, thermal=None, schedule=None):
    ctx.init_cells(soc0, tc)
    if limits:
        ctx.set_limits(**limits)
    if thermal:
        ctx.thermal_begin(**thermal)
    if schedule:
        ctx.thermal_schedule(*schedule[0], **schedule[1])


def host_loop(ctx, S, nsteps, rec=None, thermal=False):
    """The reference: nsteps times step(1) + get_state + pack_ref + set_state on a context without
    a pack.  Returns the per-step rows and the record."""
    n = ctx.n
    rows = {k: [] for k in KEYS + ("ucmd", "limiter") + (("temp", "heat") if thermal else ())}
    for _ in range(nsteps):
        o = ctx.step(1, outputs=KEYS, thermal=("temp", "heat") if thermal else None)
        scal = ctx.get_state()["scal"]
        ucmd = scal[:, S_UK].copy()
        r = pr.reduce(ucmd[None, :], S, state=rec)
        rec = {k: r[k] for k in pr.FIELDS}
        ok = ~np.isnan(ucmd)
        scal[ok, S_UK] = r["u"][0][ok]
        scal[ok, S_UK_1] = r["u"][0][ok]
        ctx.set_state({"scal": scal})
        for k in KEYS[1:] + (("temp", "heat") if thermal else ()):
            rows[k].append(o[k][0])
        rows["u"].append(r["u"][0])
        rows["ucmd"].append(ucmd)
        rows["limiter"].append(r["limiter"][0])
    out = {k: np.stack(v) if v else np.empty((0, n)) for k, v in rows.items()}
    out["rec"] = rec if rec is not None else pr.reset(n)
    return out


def pack_run(ctx, S, calls, thermal=False):
    """The code under test: pack_begin(S), then the calls' steps, rows concatenated."""
    ctx.pack_begin(S)
    parts = [ctx.step(m, outputs=KEYS, pack=("ucmd", "limiter"), thermal=("temp", "heat") if thermal else None)
             for m in calls]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["rec"] = ctx.pack_get()
    return out


def compare(got, ref, what, extra=()):
    for k in KEYS + ("ucmd", "limiter") + tuple(extra):
        same(got[k], ref[k], f"{what}: {k}")
    assert tuple(got["rec"]) == pr.FIELDS
    for k in pr.FIELDS:
        same(got["rec"][k], ref["rec"][k], f"{what}: record {k}")


def stats(ref):
    """(strings whose limiter changes during the run, share of (cell, step) pairs with ucmd != u)."""
    lim = ref["limiter"]
    differ = (ref["ucmd"] != ref["u"]) & ~(np.isnan(ref["ucmd"]) & np.isnan(ref["u"]))
    return int((lim[1:] != lim[:-1]).any(axis=0).sum()), float(differ.mean())


def pair(M, rom, n, S, nsteps, cfg=None, limits=None, env=None, calls=None, graph=False, soc0=None, tc=None, warm=0):
    """(reference loop, fused pack) on two contexts of one configuration, states included.
    warm: uncoupled steps on both before either begins."""
    with _env(**(env or {})):
        a, b = M.Context(rom, n, cfg), M.Context(rom, n, cfg)
    with a, b:
        for c in (a, b):
            setup(c, soc0, tc, limits)
            c.step(warm, outputs=())
        ref = host_loop(a, S, nsteps)
        b.set_graph(graph)
        got = pack_run(b, S, calls or (nsteps,))
        ref["state"], got["state"] = a.get_state(), b.get_state()
    return ref, got


# ---- 1. the precondition of the reference loop --------------------------------------------------
def test_state_round_trip_perturbs_nothing(M, rom):
    n, N = 300, NSTEPS
    soc0, tc, lim = inputs(n, 3)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
        one = a.step(N, outputs=KEYS)
        rows = {k: [] for k in KEYS}
        for _ in range(N):
            o = b.step(1, outputs=KEYS)
            b.set_state({"scal": b.get_state()["scal"]})
            for k in KEYS:
                rows[k].append(o[k][0])
        for k in KEYS:
            same(np.stack(rows[k]), one[k], f"step(1) + get_state + set_state x {N} vs step({N}): {k}")
        state_equal(b.get_state(), a.get_state(), "round trip")


# ---- 2. the host-driven loop equals the fused pack ----------------------------------------------
@pytest.mark.parametrize("S", sorted(SHAPES))
def test_host_loop_equals_fused_pack(M, rom, S):
    n = S * SHAPES[S]
    assert n <= 2100
    soc0, tc, lim = inputs(n, S)
    ref, got = pair(M, rom, n, S, NSTEPS, limits=lim, soc0=soc0, tc=tc)
    changed, share = stats(ref)
    print(f"S = {S}: {n} cells, {changed} of {SHAPES[S]} strings change their limiter, ucmd != u in {share:.3f}")
    # on the reference loop's output, before the comparison: the case is not vacuous
    assert changed >= 1, "no string's limiter changes during the run"
    assert share >= 0.25, f"ucmd != u in {share:.3f} of the (cell, step) pairs"
    assert got["limiter"].shape == (NSTEPS, SHAPES[S]) and got["limiter"].dtype == np.int32
    compare(got, ref, f"S = {S}")
    state_equal(got["state"], ref["state"], f"S = {S}")


# ---- 3. S = 1 is the identity -------------------------------------------------------------------
@pytest.mark.parametrize("horizon", [(5, 2), (20, 10)])
def test_series_one_is_the_identity(M, rom, horizon):
    n, N = 300, 40
    soc0, tc, lim = inputs(n, 3)
    cfg = M.make_config(Np=horizon[0], Nc=horizon[1])
    with M.Context(rom, n, cfg) as a, M.Context(rom, n, cfg) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
        plain = a.step(N, outputs=KEYS)
        got = pack_run(b, 1, (N,))
        for k in KEYS:
            same(got[k], plain[k], f"S = 1: {k}")
        same(got["ucmd"], plain["u"], "S = 1: ucmd")
        assert (got["limiter"] == 0).all() and got["limiter"].shape == (N, n)
        state_equal(b.get_state(), a.get_state(), "S = 1")
    rec = got["rec"]
    assert (rec["nlim"] == rec["steps"]).all() and (rec["steps"] == N).all()
    same(rec["headroom"], np.zeros(n), "S = 1: headroom")


# ---- 4. ties and NaN cells by construction ------------------------------------------------------
def test_ties_and_error_cells(M, rom):
    S, N = 7, 30
    n = 3 * S
    soc0, tc = np.full(n, 30.0), np.full(n, 25.0)
    soc0[S:2 * S] = np.linspace(20.0, 50.0, S)     # string 1: different cells, an error cell in the middle
    bad = S + 3
    soc0[bad] = 130.0                              # thetae < 0: in error, its outputs NaN, from its third step on
    soc0[2 * S:] = 130.0                           # string 2: error cells only
    lim = dict(Crate=np.where(np.arange(n) % 2 == 0, 1.0, 2.0))
    lim["Crate"][:S] = 2.0                         # string 0: identical cells
    # four uncoupled steps first: the cells at 130 % are in error before the strings form (the
    # two commands they give before that are thousands of amperes)
    ref, got = pair(M, rom, n, S, N, limits=lim, soc0=soc0, tc=tc, warm=4)
    compare(got, ref, "ties / NaN")
    state_equal(got["state"], ref["state"], "ties / NaN")
    # string 0: a tie at every step goes to index 0, and nothing changes
    assert (got["limiter"][:, 0] == 0).all()
    same(got["ucmd"][:, :S], got["u"][:, :S], "identical cells: ucmd == u")
    assert (got["rec"]["nlim"][:S] == np.r_[N, np.zeros(S - 1)]).all() and (got["rec"]["headroom"][:S] == 0).all()
    # string 1: the error cell is excluded and stays NaN, the others carry one current
    assert got["state"]["status"][bad] & 1
    assert np.isnan(got["u"][:, bad]).all() and np.isnan(got["ucmd"][:, bad]).all()
    assert got["rec"]["steps"][bad] == 0 and got["rec"]["nlim"][bad] == 0 and got["rec"]["headroom"][bad] == 0
    others = np.setdiff1d(np.arange(S, 2 * S), [bad])
    assert (got["u"][:, others] == got["u"][:, others[:1]]).all() and (got["limiter"][:, 1] != 3).all()
    assert (got["ucmd"][:, others] != got["u"][:, others]).any() and (got["rec"]["steps"][others] == N).all()
    # string 2: nothing to reduce
    assert (got["limiter"][:, 2] == -1).all() and np.isnan(got["u"][:, 2 * S:]).all()
    assert (got["rec"]["steps"][2 * S:] == 0).all()


# ---- 5. routes ----------------------------------------------------------------------------------
ROUTES = {
    # name: (n, S, N, make_config keywords, per-cell limits?, environment, calls, graph)
    "mb": (192, 12, 30, dict(method="MB"), True, {}, None, False),
    "mask_eta_off": (192, 12, 30, dict(constraints=(1, 1, 0)), True, {}, None, False),
    "percell_all_on": (192, 12, 30, {}, True, {}, None, False),
    "np20": (96, 12, 20, dict(Np=20, Nc=10), True, {}, None, False),
    "ekf4": (192, 12, 30, {}, False, dict(MPCEKF_QUAD=1), None, False),
    "split_cell": (192, 12, 30, {}, False, dict(MPCEKF_QUAD=0, MPCEKF_SPLIT_CELL=1), None, False),
    "graph": (192, 12, 30, {}, True, {}, (15, 15), True),
    "n_calls_of_one": (192, 12, 30, {}, True, {}, (1,) * 30, False),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(M, rom, route):
    n, S, N, kw, percell, env, calls, graph = ROUTES[route]
    soc0, tc, lim = inputs(n, S)
    if not percell:   # no set_limits (it would take the route away): the SOC0 spread alone, up to the voltage limit
        soc0, lim = np.linspace(10.0, 92.0, n)[np.random.Generator(np.random.PCG64(5)).permutation(n)], None
    ref, got = pair(M, rom, n, S, N, cfg=M.make_config(**kw), limits=lim, env=env, calls=calls, graph=graph,
                    soc0=soc0, tc=tc)
    changed, share = stats(ref)
    print(f"{route}: {changed} of {n // S} strings change their limiter, ucmd != u in {share:.3f}")
    assert share > 0, "the strings couple nothing"
    compare(got, ref, route)
    state_equal(got["state"], ref["state"], route)


def test_begin_steps_end_steps(M, rom):
    n, S = 192, 12
    soc0, tc, lim = inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as twin:
        for c in (a, b, twin):
            setup(c, soc0, tc, lim)
        ref = host_loop(a, S, 20)
        got = pack_run(b, S, (20,))
        compare(got, ref, "before the end")
        b.pack_end()
        b.pack_end()                                   # a no-op without a begin
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: pack_get"):
            b.pack_get()
        twin.set_state(b.get_state())                  # an uncoupled context started from that state
        x, y = b.step(15, outputs=KEYS), twin.step(15, outputs=KEYS)
        for k in KEYS:
            same(x[k], y[k], f"after the end: {k}")
        state_equal(b.get_state(), twin.get_state(), "after the end")
        assert (x["u"][-1].reshape(-1, S) != x["u"][-1].reshape(-1, S)[:, :1]).any()   # every cell on its own again


# ---- 6. with the thermal model and a schedule ---------------------------------------------------
def test_thermal_model_and_schedule(M, rom):
    import test_gpu_thermal as tg
    n, S, N = 128, 16, 50
    p = tg.params(n)
    rng = np.random.Generator(np.random.PCG64(0x7AC6))
    p["soc0"] = rng.uniform(10.0, 60.0, n)
    p["Cth"] = rng.uniform(20.0, 60.0, n)              # J/K: kelvins within the run
    ocv = M.thermal_ocv(rom)
    th = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=ocv)
    # three derating maps over 20..40 degC, one per cell in turn: Crate falls as the cell warms
    grid = np.linspace(0.0, 1.0, 5)
    sched = ((20.0, 40.0), dict(sets=(np.arange(n) % 3).astype(np.int32),
                                Crate=np.stack([2.0 - 0.8 * grid, 1.6 - 0.5 * grid, 1.2 - 0.3 * grid])))
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, p["soc0"], p["T0"], None, th, sched)
        uk0 = b.get_scalars(("uk",))["uk"].copy()
        ref = host_loop(a, S, N, thermal=True)
        b.pack_begin(S)
        got = b.step(N, outputs=KEYS, pack=("ucmd", "limiter"), thermal=("temp", "heat"), obs=("negSOC",))
        got["rec"] = b.pack_get()
        compare(got, ref, "thermal", extra=("temp", "heat"))
        ra, rb = a.thermal_get(), b.thermal_get()
        for k in ra:
            same(rb[k], ra[k], f"thermal record {k}")
        state_equal(b.get_state(), a.get_state(), "thermal")
        socn_end = b.get_scalars(("SOCnAvg",))["SOCnAvg"].copy()
    changed, share = stats(ref)
    print(f"thermal: {changed} of {n // S} strings change their limiter, ucmd != u in {share:.3f}")
    assert share >= 0.25
    # heat is i (U - v) of the applied current: the header's recurrence with u, not ucmd, as i
    temp, heat, _, _ = tg.restate(rom, p, ocv, p["T0"], uk0, got["u"], got["v"], got["obs"]["negSOC"], socn_end)
    same(temp, got["temp"], "temp vs the recurrence on the applied current")
    same(heat, got["heat"], "heat vs the recurrence on the applied current")
    _, other, _, _ = tg.restate(rom, p, ocv, p["T0"], uk0, got["ucmd"], got["v"], got["obs"]["negSOC"], socn_end)
    assert (other[1:] != heat[1:]).mean() >= 0.25                    # the commands would have heated otherwise


# ---- 7. with the summary ------------------------------------------------------------------------
def test_step_summary_on_a_pack_context(M, rom):
    n, S, N = 192, 12, 70                               # 70 steps: a full 64-row window and a partial one
    soc0, tc, lim = inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
            c.pack_begin(S)
        traj = a.step(N, outputs=KEYS, pack=("ucmd",))
        b.summary_begin()
        b.step_summary(N)
        got = b.get_summary()
        ref = sr.reduce(traj)
        sr.same_record(got, ref, "summary", fields=[k for k in sr.FIELDS if not k.startswith("obs_")])
        ra, rb = a.pack_get(), b.pack_get()
        for k in pr.FIELDS:
            same(rb[k], ra[k], f"pack record {k}")
        state_equal(b.get_state(), a.get_state(), "summary")
    assert (traj["ucmd"] != traj["u"]).mean() >= 0.25
    same(got["u_last"], traj["u"][-1], "u_last is the applied current")


def test_wrappers_pass_the_pack_through(M, rom):
    n, S, N = 36, 12, 12
    soc0, tc, lim = inputs(n, S)
    out = M.runMPC(rom, soc0, tc, N, limits=lim, pack=dict(series=S))
    assert out["limiter"].shape == (N, n // S) and out["ucmd"].shape == (N, n) and tuple(out["pack"]) == pr.FIELDS
    r = pr.reduce(out["ucmd"], S)
    for k in ("u", "limiter"):
        same(out[k], r[k], f"runMPC: {k}")
    s = M.run_summary(rom, soc0, tc, N, limits=lim, pack=dict(series=S), chunk=5)
    for k in pr.FIELDS:
        same(s["pack"][k], out["pack"][k], f"run_summary: pack record {k}")
        same(out["pack"][k], r[k], f"runMPC: pack record {k}")
    same(s["u_last"], out["u"][-1], "run_summary: u_last")


# ---- 8. refusals --------------------------------------------------------------------------------
def test_refusals_change_nothing(M, rom):
    n, S = 36, 12
    soc0, tc, lim = inputs(n, S)
    with M.Context(rom, n) as ctx:
        setup(ctx, soc0, tc, lim)
        ctx.step(3, outputs=())
        st0 = ctx.get_state()
        # without a begin
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_pack: call mpcekf_pack_begin first"):
            ctx.step(2, pack=("ucmd", "limiter"))
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_pack"):
            ctx.step(2, pack=())
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: pack_get"):
            ctx.pack_get()
        for bad in (0, -3, 5, 37, 72):
            with pytest.raises(M.MpcekfError, match=f"mpcekf error -1: pack_begin: series = {bad}"):
                ctx.pack_begin(bad)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: pack_get"):    # a refused begin began nothing
            ctx.pack_get()
        state_equal(ctx.get_state(), st0, "refused without a begin")
        # with a begin: a bad series, temp / heat rows without a model
        ctx.pack_begin(S)
        ctx.step(5, outputs=())
        st1, rec1 = ctx.get_state(), ctx.pack_get()
        assert (rec1["steps"] == 5).all()
        for bad in (0, 5, -1):
            with pytest.raises(M.MpcekfError, match=f"mpcekf error -1: pack_begin: series = {bad}"):
                ctx.pack_begin(bad)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_pack: temp / heat rows"):
            ctx.step(2, pack=("ucmd",), thermal=("temp",))
        state_equal(ctx.get_state(), st1, "refused with a begin")
        for k in pr.FIELDS:
            same(ctx.pack_get()[k], rec1[k], f"refused with a begin: record {k}")
        o = ctx.step(2, outputs=KEYS, pack="limiter")           # the refused begins left series = S in force
        assert o["limiter"].shape == (2, n // S) and "ucmd" not in o
        assert (o["u"].reshape(2, -1, S) == o["u"].reshape(2, -1, S)[:, :, :1]).all()
        ctx.pack_begin(S // 2)                                  # a second begin replaces the first, record reset
        assert all((v == 0).all() for v in ctx.pack_get().values())
        o = ctx.step(1, outputs=KEYS, pack="limiter")
        assert o["limiter"].shape == (1, 2 * n // S)
