"""GPU: passive balancing of pack strings along the fused loop (mpcekf_balance_begin / _get /
_end, mpcekf_step_ex_balance; k_pack_bal in k_pack's place in every fused step).

The reference everywhere is the host-driven loop the feature replaces, on a second context that
has neither pack nor balancer: per step, step(1) with the soc row, get_state, tests/balance_ref.py
(the header's rule in plain Python) on the uk column and that soc row, uk / uk_1 written back with
set_state({"scal": ...}).  Every comparison is bitwise (a NaN equals a NaN).  Nothing expected
comes from the code under test.  (The loop's precondition, that the get_state / set_state round
trip perturbs nothing, is test_gpu_pack.py's first test.)

  1. host loop == fused balancer over S in {2, 3, 5, 64, 96, 100, 256, 257, 1000}, compensate 0 / 1
  2. identities: i_bleed = 0, an unreachable dz_on, S = 1
  3. NaN commands by construction, a string of NaN commands only
  4. routes (MB, a mask, Np = 20, k_ekf4, the split k_cell, graph replay, call splitting, end)
  5. with the thermal model + schedule (+ links), step_summary, aging, termination / step_until
  6. refusals
"""
import numpy as np
import pytest

import balance_ref as br
import pack_ref as pr
import summary_ref as sr
import term_ref as tr
import test_gpu_pack as tp
from test_gpu_pack import KEYS, NSTEPS, SHAPES, S_UK, S_UK_1, _env, same, setup, state_equal

pytestmark = pytest.mark.gpu

ROWS = ("ucmd", "limiter", "bleed", "zmin")
I_1C = 30.0          # A: about the 1 C current of the synthetic ROM's cell (29.86 A; its soc rises 0.2 % per step)
DZ_ON, DZ_OFF = 0.01, 0.005


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def inputs(n, S, seed=0xBA1A):
    """test_gpu_pack.py's inputs() (an in-string SOC0 spread of tens of percent, so most cells sit
    more than dz_on = 0.01 above their string's smallest soc from step 1) with a per-cell bleed
    current among 0, 0.05, 0.1, 0.2 of the 1 C current (the string's first cell 0.1), and the
    string's second cell, by string number g, one of
      A (g % 8 == 0)  3 % above the lowest of the others, bleeding 1 C: the gap closes 0.2 % per
                      step through dz_off within the run, the bleeder goes off;
      B (g % 8 == 1)  1.75 % above the lowest of the others, bleeding 5 C: the gap closes 1 % per
                      step, 0.75 % (held on) and then below zero: the string's arg-min from then on;
      C (otherwise)   3 % below the lowest of the others, at Crate 1: the arg-min; the string's
                      first cell, whose command ties with it, bleeds, so with compensate the
                      limiter is not the pack's.
    The large bleeds exercise the kernel; a realistic 0.1 A closes no gap in 40 steps.
    The reference loop under these inputs, 40 steps: see test_host_loop_equals_fused_balancer."""
    soc0, tc, lim = tp.inputs(n, S)
    rng = np.random.Generator(np.random.PCG64(seed + S))
    idx, g = np.arange(n) % S, np.arange(n) // S
    ib = rng.choice(np.array([0.0, 0.05, 0.1, 0.2]), n) * I_1C
    ib[idx == 0] = 0.1 * I_1C
    others = np.where(idx == 1, np.inf, soc0).reshape(-1, S).min(axis=1)
    second = idx == 1
    kind = np.where(g % 8 == 0, 0, np.where(g % 8 == 1, 1, 2))
    soc0[second] = (others + np.array([3.0, 1.75, -3.0])[kind[second]])
    ib[second] = np.array([1.0, 5.0, 0.0])[kind[second]] * I_1C
    lim["Crate"][second & (kind == 2)] = 1.0
    return soc0, tc, lim, (ib, np.full(n, DZ_ON), np.full(n, DZ_OFF))


def host_loop(ctx, S, nsteps, par, comp, st=None, thermal=False, packed=False, stop=None, tst=None, T=None):
    """The reference: nsteps times step(1) + get_state + (term_ref +) balance_ref + set_state on a
    context without a balancer.  packed: the context is a balancer-free pack itself (for the
    links): the cells' own commands are its ucmd row.  stop: term_begin's keywords, the rule of
    tests/term_ref.py before the balancer's.  Returns the per-step rows and the records."""
    n = ctx.n
    th = ("temp", "heat") if thermal else ()
    rows = {k: [] for k in KEYS + ROWS + th}
    tst = tr.reset(n) if stop is not None and tst is None else tst
    for _ in range(nsteps):
        o = ctx.step(1, outputs=KEYS, thermal=th or None, pack=("ucmd",) if packed else None)
        scal = ctx.get_state()["scal"]
        own = o["ucmd"][0].copy() if packed else scal[:, S_UK].copy()
        if stop is not None:
            own, tst = tr.step(tst, o["soc"][0], own, o["temp"][0] if thermal else T, series=S, **stop)
        r = br.step(own[None, :], o["soc"], S, *par, comp, state=st)
        st = {k: r[k] for k in br.PACK_FIELDS + br.FIELDS + ("on",)}
        ok = ~np.isnan(own)
        scal[ok, S_UK] = r["u"][0][ok]
        scal[ok, S_UK_1] = r["u"][0][ok]
        ctx.set_state({"scal": scal})
        for k in KEYS[1:] + th:
            rows[k].append(o[k][0])
        rows["ucmd"].append(own)
        for k in ("u", "limiter", "bleed", "zmin"):
            rows[k].append(r[k][0])
    out = {k: np.stack(v) if v else np.empty((0, n)) for k, v in rows.items()}
    out["st"], out["tst"] = st if st is not None else br.reset(n), tst
    return out


def fused(ctx, S, calls, par, comp, thermal=False, begin=True):
    """The code under test: pack_begin(S), balance_begin, then the calls' steps, rows concatenated."""
    if begin:
        ctx.pack_begin(S)
        ctx.balance_begin(*par, compensate=bool(comp))
    parts = [ctx.step(m, outputs=KEYS, pack=ROWS, thermal=("temp", "heat") if thermal else None) for m in calls]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["pack"], out["balance"] = ctx.pack_get(), ctx.balance_get()
    return out


def compare(got, ref, what, extra=()):
    for k in KEYS + ROWS + tuple(extra):
        same(got[k], ref[k], f"{what}: {k}")
    assert tuple(got["pack"]) == pr.FIELDS and tuple(got["balance"]) == tuple(br.LIB_NAMES.values())
    for k in pr.FIELDS:
        same(got["pack"][k], ref["st"][k], f"{what}: pack record {k}")
    for k in br.FIELDS:
        same(got["balance"][br.LIB_NAMES[k]], ref["st"][k], f"{what}: balance record {k}")


def stats(ref, S):
    """On the reference loop's output: (share of (cell, step) pairs that bleed, cells that switch
    on -> off after the first step, strings whose arg-min cell changes, (string, step) pairs whose
    limiter is not pack_ref's on the same commands)."""
    b = ref["bleed"] > 0
    off = int((b[:-1] & ~b[1:]).any(axis=0).sum())
    N, n = ref["soc"].shape
    z = np.where(np.isnan(ref["ucmd"]) | np.isnan(ref["soc"]), np.inf, ref["soc"]).reshape(N, -1, S)
    amin = z.argmin(axis=2)
    moved = int((amin[1:] != amin[:-1]).any(axis=0).sum())
    other = int((ref["limiter"] != pr.reduce(ref["ucmd"], S)["limiter"]).sum())
    return float(b.mean()), off, moved, other


def pair(M, rom, n, S, nsteps, par, comp, cfg=None, limits=None, env=None, calls=None, graph=False, soc0=None, tc=None,
         warm=0):
    """(reference loop, fused balancer) on two contexts of one configuration, states included."""
    with _env(**(env or {})):
        a, b = M.Context(rom, n, cfg), M.Context(rom, n, cfg)
    with a, b:
        for c in (a, b):
            setup(c, soc0, tc, limits)
            c.step(warm, outputs=())
        ref = host_loop(a, S, nsteps, par, comp)
        b.set_graph(graph)
        got = fused(b, S, calls or (nsteps,), par, comp)
        ref["state"], got["state"] = a.get_state(), b.get_state()
    return ref, got


# ---- 1. the host-driven loop equals the fused balancer ------------------------------------------
@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("S", sorted(SHAPES))
def test_host_loop_equals_fused_balancer(M, rom, S, comp):
    """Achieved on the reference loop (40 steps; the same for both compensate values except the
    last figure, which is 0 by construction with compensate = 0), S: share of (cell, step) pairs
    bleeding / cells that switch on -> off / strings whose arg-min cell changes / (string, step)
    pairs whose limiter is not pack_ref's:
      2: 0.416 / 50 / 19 of 200 / 5850 of 8000      3: 0.522 / 30 / 14 of 120 / 1689 of 4800
      5: 0.630 / 19 / 9 of 70 / 607 of 2800         64: 0.741 / 2 / 1 of 6 / 99 of 240
      96: 0.749 / 3 / 1 of 5 / 62 of 200            100: 0.751 / 3 / 1 of 5 / 55 of 200
      256: 0.736 / 8 / 1 of 3 / 49 of 120           257: 0.776 / 2 / 1 of 3 / 49 of 120
      1000: 0.732 / 11 / 1 of 2 / 41 of 80"""
    n = S * SHAPES[S]
    assert n <= 2100
    soc0, tc, lim, par = inputs(n, S)
    ref, got = pair(M, rom, n, S, NSTEPS, par, comp, limits=lim, soc0=soc0, tc=tc)
    share, off, moved, other = stats(ref, S)
    print(f"S = {S}, compensate = {comp}: {n} cells, bleeding in {share:.3f} of the (cell, step) pairs, {off} cells "
          f"switch on -> off, {moved} of {SHAPES[S]} strings change their arg-min cell, limiter != pack_ref's in "
          f"{other} of {NSTEPS * SHAPES[S]} (string, step) pairs")
    # on the reference loop's output, before the comparison: the case is not vacuous
    assert share >= 0.25, f"bleeding in {share:.3f} of the (cell, step) pairs"
    assert off >= 1, "no cell switches on -> off after the first step"
    assert moved >= 1, "no string's arg-min cell changes during the run"
    if comp:
        assert other >= 1, "the limiter is pack_ref's everywhere"
    assert got["zmin"].shape == (NSTEPS, SHAPES[S]) and got["bleed"].shape == (NSTEPS, n)
    compare(got, ref, f"S = {S}, compensate = {comp}")
    state_equal(got["state"], ref["state"], f"S = {S}")


# ---- 2. identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_bleeder", "unreachable", "series_one"])
def test_identities(M, rom, case):
    n, S, N = 300, 1 if case == "series_one" else 12, NSTEPS
    soc0, tc, lim, par = inputs(n, 12)
    if case == "no_bleeder":
        par = (np.zeros(n),) + par[1:]
    elif case == "unreachable":
        par = (par[0], np.full(n, 5.0), np.full(n, 2.5))
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
        a.pack_begin(S)
        plain = a.step(N, outputs=KEYS, pack=("ucmd", "limiter"))
        got = fused(b, S, (N,), par, 1)
        for k in KEYS + ("ucmd", "limiter"):
            same(got[k], plain[k], f"{case}: {k}")
        for k in pr.FIELDS:
            same(got["pack"][k], a.pack_get()[k], f"{case}: pack record {k}")
        state_equal(b.get_state(), a.get_state(), case)
    same(got["bleed"], np.where(np.isnan(plain["ucmd"]), np.nan, 0.0), f"{case}: bleed")
    rec = got["balance"]
    assert (rec["steps_on"] == 0).all() and (rec["q_bleed"] == 0).all() and (rec["steps"] == N).all()
    if case == "series_one":
        same(got["zmin"], plain["soc"], "S = 1: zmin is the cell's own soc")
        same(rec["dz_max"], np.zeros(n), "S = 1: d = 0")
    if case == "no_bleeder":
        assert rec["switches"].sum() > 0                 # the flags switch all the same


# ---- 3. NaN commands by construction ------------------------------------------------------------
def test_nan_commands_and_an_all_nan_string(M, rom):
    S, N = 7, 30
    n = 3 * S
    soc0, tc = np.full(n, 30.0), np.full(n, 25.0)
    soc0[:S] = np.linspace(25.0, 40.0, S)
    soc0[S:2 * S] = np.linspace(20.0, 50.0, S)     # string 1: an error cell in the middle
    bad = S + 3
    soc0[bad] = 130.0                              # thetae < 0: in error, its outputs NaN, from its third step on
    soc0[2 * S:] = 130.0                           # string 2: error cells only
    lim = dict(Crate=np.where(np.arange(n) % 2 == 0, 1.0, 2.0))
    par = (np.full(n, 0.25 * I_1C), np.full(n, DZ_ON), np.full(n, DZ_OFF))
    ref, got = pair(M, rom, n, S, N, par, 1, limits=lim, soc0=soc0, tc=tc, warm=4)
    compare(got, ref, "NaN cells")
    state_equal(got["state"], ref["state"], "NaN cells")
    assert got["state"]["status"][bad] & 1
    assert np.isnan(got["u"][:, bad]).all() and np.isnan(got["bleed"][:, bad]).all()
    rec = got["balance"]
    assert rec["steps"][bad] == 0 and rec["steps_on"][bad] == 0 and np.isnan(rec["dz_last"][bad])
    assert (got["limiter"][:, 1] != 3).all() and (got["bleed"][:, S:2 * S] > 0).any()
    assert (got["limiter"][:, 2] == -1).all() and np.isnan(got["u"][:, 2 * S:]).all()
    assert np.isnan(got["zmin"][:, 2]).all()
    assert (got["balance"]["steps"][2 * S:] == 0).all() and np.isnan(got["balance"]["dz_max"][2 * S:]).all()


# ---- 4. routes ----------------------------------------------------------------------------------
ROUTES = {
    # name: (n, S, N, make_config keywords, per-cell limits?, environment, calls, graph)
    "mb": (240, 12, 30, dict(method="MB"), True, {}, None, False),
    "mask_eta_off": (240, 12, 30, dict(constraints=(1, 1, 0)), True, {}, None, False),
    "np20": (204, 12, 20, dict(Np=20, Nc=10), True, {}, None, False),
    "ekf4": (240, 12, 30, {}, False, dict(MPCEKF_QUAD=1), None, False),
    "split_cell": (240, 12, 30, {}, False, dict(MPCEKF_QUAD=0, MPCEKF_SPLIT_CELL=1), None, False),
    "graph": (240, 12, 40, {}, True, {}, (10, 10, 10, 10), True),
    "calls_7_1_32": (240, 12, 40, {}, True, {}, (7, 1, 32), False),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(M, rom, route):
    n, S, N, kw, percell, env, calls, graph = ROUTES[route]
    soc0, tc, lim, par = inputs(n, S)
    if not percell:   # no set_limits (it would take the route away): the SOC0 spread alone
        lim = None
    ref, got = pair(M, rom, n, S, N, par, 1, cfg=M.make_config(**kw), limits=lim, env=env, calls=calls, graph=graph,
                    soc0=soc0, tc=tc)
    share, off, moved, other = stats(ref, S)
    print(f"{route}: bleeding in {share:.3f}, {off} cells switch off, {moved} strings change their arg-min, "
          f"limiter != pack_ref's in {other}")
    assert share > 0.1, "nothing bleeds"
    compare(got, ref, route)
    state_equal(got["state"], ref["state"], route)


def test_begin_steps_end_steps(M, rom):
    n, S = 240, 12
    soc0, tc, lim, par = inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as twin:
        for c in (a, b, twin):
            setup(c, soc0, tc, lim)
        ref = host_loop(a, S, 20, par, 1)
        got = fused(b, S, (20,), par, 1)
        compare(got, ref, "before the end")
        b.balance_end()
        b.balance_end()                                # a no-op without a begin
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: balance_get"):
            b.balance_get()
        twin.set_state(b.get_state())                  # a balancer-free pack started from that state
        twin.pack_begin(S)
        x, y = b.step(15, outputs=KEYS, pack=("ucmd", "limiter")), twin.step(15, outputs=KEYS, pack=("ucmd", "limiter"))
        for k in x:
            same(x[k], y[k], f"after the end: {k}")
        state_equal(b.get_state(), twin.get_state(), "after the end")
        b.balance_begin(*par)                          # pack_end ends a balancer too
        b.pack_end()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: balance_get"):
            b.balance_get()
        # pack_begin with another S keeps the balancer: parameters and flags are per cell
        b.pack_begin(S)
        b.balance_begin(*par)
        b.step(3, outputs=())
        b.pack_begin(S // 2)
        assert (b.balance_get()["steps"] == 3).all()
        o = b.step(2, outputs=KEYS, pack=ROWS)
        assert o["zmin"].shape == (2, 2 * n // S)


# ---- 5. with the other pack features ------------------------------------------------------------
def _thermal(M, rom, n):
    import test_gpu_thermal as tg
    p = tg.params(n)
    rng = np.random.Generator(np.random.PCG64(0x7AC6))
    p["Cth"] = rng.uniform(20.0, 60.0, n)              # J/K: kelvins within the run
    th = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom))
    grid = np.linspace(0.0, 1.0, 5)
    sched = ((20.0, 40.0), dict(sets=(np.arange(n) % 3).astype(np.int32),
                                Crate=np.stack([2.0 - 0.8 * grid, 1.6 - 0.5 * grid, 1.2 - 0.3 * grid])))
    return p, th, sched, rng


@pytest.mark.parametrize("links", [False, True])
def test_thermal_model_schedule_and_links(M, rom, links):
    n, S, N = 192, 16, 40
    soc0, _, _, par = inputs(n, S)
    p, th, sched, rng = _thermal(M, rom, n)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, p["T0"], None, th, sched)
        if links:                                      # links need strings: the reference is a balancer-free pack
            r_link = rng.uniform(0.5, 3.0, n)
            a.pack_begin(S)
            a.thermal_couple(r_link)
        ref = host_loop(a, S, N, par, 1, thermal=True, packed=links)
        b.pack_begin(S)
        if links:
            b.thermal_couple(r_link)
        b.balance_begin(*par)
        got = fused(b, S, (N,), par, 1, thermal=True, begin=False)
        if links:                                      # the reference's own pack record counted its own reduction
            for k in ROWS + KEYS + ("temp", "heat"):
                same(got[k], ref[k], f"links: {k}")
            for k in br.FIELDS:
                same(got["balance"][br.LIB_NAMES[k]], ref["st"][k], f"links: balance record {k}")
            for k, v in a.thermal_couple_get().items():
                same(b.thermal_couple_get()[k], v, f"links: couple record {k}")
        else:
            compare(got, ref, "thermal", extra=("temp", "heat"))
        for k, v in a.thermal_get().items():
            same(b.thermal_get()[k], v, f"thermal record {k}")
        state_equal(b.get_state(), a.get_state(), "thermal")
    assert stats(ref, S)[0] >= 0.25


def test_step_summary(M, rom):
    n, S, N = 240, 12, 70                               # 70 steps: a full 64-row window and a partial one
    soc0, tc, lim, par = inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
        ref = host_loop(a, S, N, par, 1)
        b.pack_begin(S)
        b.balance_begin(*par)
        b.summary_begin()
        b.step_summary(30)
        b.step_summary(40)
        got = b.get_summary()
        sr.same_record(got, sr.reduce(ref), "summary", fields=[k for k in sr.FIELDS if not k.startswith("obs_")])
        rec, pk = b.balance_get(), b.pack_get()
        for k in br.FIELDS:
            same(rec[br.LIB_NAMES[k]], ref["st"][k], f"summary: balance record {k}")
        for k in pr.FIELDS:
            same(pk[k], ref["st"][k], f"summary: pack record {k}")
        state_equal(b.get_state(), a.get_state(), "summary")
    same(got["u_last"], ref["u"][-1], "u_last is the cell's own applied current")


def test_aging_estimate_source(M, rom):
    import test_gpu_aging as ta
    n, S, N = 240, 12, 30
    soc0, tc, lim, par = inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
            c.aging_begin(ta.reactions(n, 2), sources=("est",))
        ref = host_loop(a, S, N, par, 1)
        got = fused(b, S, (N,), par, 1)
        compare(got, ref, "aging")
        ra, rb = a.aging_record(), b.aging_record()
        assert str(sorted(ra)) == str(sorted(rb))
        _same_tree(rb, ra, "aging record")
        state_equal(b.get_state(), a.get_state(), "aging")


def _same_tree(x, y, what):
    if isinstance(x, dict):
        assert set(x) == set(y), what
        for k in x:
            _same_tree(x[k], y[k], f"{what}: {k}")
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), what
        for i, (p, q) in enumerate(zip(x, y)):
            _same_tree(p, q, f"{what}: {i}")
    else:
        same(np.asarray(x), np.asarray(y), what)


def test_termination_and_step_until(M, rom):
    """A latched cell's string rests at 0 A while its bleeding cells get +b_c; step_until runs on
    NULL outputs, so k_term and k_pack_bal read the context's own soc row."""
    n, S, N = 240, 12, 40
    soc0, tc, lim, par = inputs(n, S)
    # each string's highest cell stops 2 % above where it starts (the synthetic ROM's soc rises a
    # few tenths of a percent per step: within the run), every third string never
    top = soc0.reshape(-1, S).argmax(axis=1) + S * np.arange(n // S)
    soc_stop = np.full(n, 2.0)
    soc_stop[top] = soc0[top] / 100.0 + 0.02
    soc_stop[top[::3]] = 2.0
    stop = dict(soc_stop=soc_stop)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as c3:
        for c in (a, b, c3):
            setup(c, soc0, tc, lim)
        ref = host_loop(a, S, N, par, 1, stop=stop, T=tc)
        for c in (b, c3):
            c.pack_begin(S)
            c.balance_begin(*par)
            c.term_begin(**stop)
        got = fused(b, S, (7, 1, 32), par, 1, begin=False)
        latched = ref["tst"]["state"] == tr.LATCHED
        print(f"termination: {int(latched.sum())} cells latched, {int((ref['tst']['state'] == tr.OPEN).sum())} open")
        assert latched.reshape(-1, S).all(axis=1).sum() >= 2 and (ref["tst"]["state"] == tr.OPEN).any()
        # on the reference: a resting string (limiter's e = +0.0) whose bleeding cells get +b
        rest = np.repeat(ref["zmin"] == ref["zmin"], S, axis=1) & (ref["ucmd"] == 0) & (ref["bleed"] > 0)
        assert rest.any() and (ref["u"][rest] == ref["bleed"][rest]).all()
        compare(got, ref, "termination")
        for k in tr.FIELDS:
            same(b.term_get()[k], tr.record(ref["tst"])[k], f"termination: term record {k}")
        state_equal(b.get_state(), a.get_state(), "termination")
        run, left = c3.step_until(N, chunk=8)                # no cell-free stop here: the cap
        assert run == N and left == int((ref["tst"]["state"] == tr.OPEN).sum())
        for k in br.FIELDS:
            same(c3.balance_get()[br.LIB_NAMES[k]], ref["st"][k], f"step_until: balance record {k}")
        state_equal(c3.get_state(), a.get_state(), "step_until")


def test_wrappers_pass_the_balancer_through(M, rom):
    n, S, N = 36, 12, 12
    soc0, tc, lim, par = inputs(n, S)
    bal = dict(i_bleed=par[0], dz_on=DZ_ON, dz_off=DZ_OFF, compensate=True)
    out = M.runMPC(rom, soc0, tc, N, limits=lim, pack=dict(series=S, balance=bal))
    r = br.step(out["ucmd"], out["soc"], S, *par, 1)
    for k in ("u", "limiter", "bleed", "zmin"):
        same(out[k], r[k], f"runMPC: {k}")
    s = M.run_summary(rom, soc0, tc, N, limits=lim, pack=dict(series=S, balance=bal), chunk=5)
    for k in br.FIELDS:
        same(out["balance"][br.LIB_NAMES[k]], r[k], f"runMPC: balance record {k}")
        same(s["balance"][br.LIB_NAMES[k]], r[k], f"run_summary: balance record {k}")
    same(s["u_last"], out["u"][-1], "run_summary: u_last")


# ---- 6. refusals --------------------------------------------------------------------------------
def test_refusals_change_nothing(M, rom):
    n, S = 36, 12
    soc0, tc, lim, par = inputs(n, S)
    with M.Context(rom, n) as ctx:
        setup(ctx, soc0, tc, lim)
        ctx.step(3, outputs=())
        st0 = ctx.get_state()
        # no pack
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: balance_begin: call mpcekf_pack_begin first"):
            ctx.balance_begin(*par)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: balance_get"):
            ctx.balance_get()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_balance: call mpcekf_balance_begin first"):
            ctx.step(2, pack=ROWS)
        state_equal(ctx.get_state(), st0, "refused without a pack")
        # a pack, no balancer
        ctx.pack_begin(S)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_balance: call mpcekf_balance_begin first"):
            ctx.step(2, pack=("bleed",))
        state_equal(ctx.get_state(), st0, "refused without a balancer")
        assert (ctx.pack_get()["steps"] == 0).all()
        # bad parameters, past the wrapper's own checks: the library refuses them itself
        ctx.balance_begin(*par)
        ctx.step(5, outputs=())
        st1, rec1, pk1 = ctx.get_state(), ctx.balance_get(), ctx.pack_get()
        assert (rec1["steps"] == 5).all() and rec1["steps_on"].sum() > 0
        L = ctx.L
        lib = M._lib
        for row, v, msg in ((0, -0.1, "i_bleed"), (0, np.nan, "i_bleed"), (1, 0.0, "dz_on"), (1, np.nan, "dz_on"),
                            (2, -0.001, "dz_off"), (2, 0.02, "dz_off"), (2, np.nan, "dz_off")):
            p = np.ascontiguousarray(np.stack(par))
            p[row, n - 1] = v
            assert L.mpcekf_balance_begin(ctx.h, lib.dptr(p), 1) == -1 and msg.encode() in L.mpcekf_last_error()
        p = np.ascontiguousarray(np.stack(par))
        for comp in (2, -1):
            assert L.mpcekf_balance_begin(ctx.h, lib.dptr(p), comp) == -1
        assert L.mpcekf_balance_begin(ctx.h, None, 1) == -1
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_balance: temp / heat rows"):
            ctx.step(2, pack=("bleed",), thermal=("temp",))
        state_equal(ctx.get_state(), st1, "refused with a balancer")
        for k in rec1:
            same(ctx.balance_get()[k], rec1[k], f"refused with a balancer: balance record {k}")
        for k in pk1:
            same(ctx.pack_get()[k], pk1[k], f"refused with a balancer: pack record {k}")
        ctx.balance_begin(*par, compensate=False)          # a second begin replaces the first, record reset
        rec = ctx.balance_get()
        assert all((rec[k] == 0).all() for k in ("steps_on", "q_bleed", "switches", "steps"))
        assert np.isnan(rec["dz_max"]).all() and np.isnan(rec["dz_last"]).all()
