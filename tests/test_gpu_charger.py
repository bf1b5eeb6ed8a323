"""GPU: charger limits on pack strings along the fused loop (mpcekf_charger_begin / _get / _end,
mpcekf_step_ex_charger; k_charger in k_pack's or k_pack_bal's place in every fused step).

The reference everywhere is the host-driven loop the feature replaces, on a second context that
has no pack: per step, step(1) with the soc row, get_state, tests/charger_ref.py (the header's rule
in plain Python, on top of pack_ref / balance_ref) on the uk, vk and soc columns, uk / uk_1 written
back with set_state({"scal": ...}).  Every comparison is bitwise (a NaN equals a NaN).  Nothing
expected comes from the code under test.  (The loop's precondition, that the get_state / set_state
round trip perturbs nothing, is test_gpu_pack.py's first test.)  The caps are fractions of the
largest current and power a cap-free reference loop on the same inputs shows, per string.

  1. host loop == fused charger over S in {1, 2, 3, 5, 64, 96, 100, 256, 257, 1000}, without a
     balancer and with one at compensate 0 / 1
  2. identities: both caps NaN / +inf against the charger-free pack or balancer
  3. NaN cells by construction, a string of NaN commands only
  4. routes (MB, a mask, Np = 20, k_ekf4, the split k_cell, graph replay, call splitting)
  5. with the thermal model + schedule (+ links), step_summary, aging, termination / step_until
  6. begin -> end -> begin, refusals, the wrappers
"""
import numpy as np
import pytest

import balance_ref as br
import charger_ref as cr
import pack_ref as pr
import summary_ref as sr
import term_ref as tr
import test_gpu_balance as tb
from test_gpu_pack import KEYS, S_UK, S_UK_1, _env, same, setup, state_equal

pytestmark = pytest.mark.gpu

S_VK = 7             # MPCEKF_S_VK
NSTEPS = 24
ROWS = ("ucmd", "limiter", "vstr", "istr", "capby")
BROWS = ("bleed", "zmin")
# S -> strings: test_gpu_pack.py's shapes (two blocks or more, strings across wave boundaries
# wherever 64 % S != 0, partial tiles at 257 and 1000) and S = 1 on three blocks
SHAPES = {1: 600, 2: 200, 3: 120, 5: 70, 64: 6, 96: 5, 100: 5, 256: 3, 257: 3, 1000: 2}
NOCAP = (np.nan, np.nan)


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def host_loop(ctx, S, nsteps, chg, bal=None, st=None, thermal=False, packed=False, stop=None, tst=None, T=None):
    """The reference: nsteps times step(1) + get_state + (term_ref +) charger_ref + set_state on a
    context without a charger.  chg: (i_max, p_max); bal: None or balance_ref's (i_bleed, dz_on,
    dz_off, compensate).  packed: the context is a charger-free pack itself (for the links): the
    cells' own commands are its ucmd row.  Returns the per-step rows and the records."""
    n = ctx.n
    th = ("temp", "heat") if thermal else ()
    rows = {k: [] for k in KEYS + ROWS + BROWS + th + ("vk", "mraw")}
    tst = tr.reset(n) if stop is not None and tst is None else tst
    for _ in range(nsteps):
        o = ctx.step(1, outputs=KEYS, thermal=th or None, pack=("ucmd",) if packed else None)
        scal = ctx.get_state()["scal"]
        own = o["ucmd"][0].copy() if packed else scal[:, S_UK].copy()
        vk = scal[:, S_VK].copy()
        if stop is not None:
            own, tst = tr.step(tst, o["soc"][0], own, o["temp"][0] if thermal else T, series=S, **stop)
        r = cr.step(own[None, :], o["soc"], vk[None, :], S, *chg, balance=bal, state=st)
        st = r["st"]
        ok = ~np.isnan(own)
        scal[ok, S_UK] = r["u"][0][ok]
        scal[ok, S_UK_1] = r["u"][0][ok]
        ctx.set_state({"scal": scal})
        for k in KEYS[1:] + th:
            rows[k].append(o[k][0])
        rows["ucmd"].append(own)
        rows["vk"].append(vk)
        for k in ("u", "limiter", "vstr", "istr", "capby", "mraw") + (BROWS if bal is not None else ()):
            rows[k].append(r[k][0])
    out = {k: np.stack(v) for k, v in rows.items() if v}
    out["st"], out["tst"] = st if st is not None else cr.reset(n, S, bal is not None), tst
    return out


def thresholds(free, fr=((0.8, 1.5), (1.5, 0.8), (0.95, 0.95))):
    """(i_max, p_max) per string from a cap-free reference loop: fractions, by string number, of
    the largest |m_g| and the largest V_g |m_g| that loop shows for the string while it charges (a
    discharging string, as a 5 C bleeder without compensation makes one, is never capped)."""
    m, V = np.where(free["mraw"] < 0, -free["mraw"], np.nan), free["vstr"]
    im, pm = np.nanmax(m, axis=0), np.nanmax(V * m, axis=0)
    g = np.arange(im.size) % len(fr)
    f = np.array(fr)
    return f[g, 0] * im, f[g, 1] * pm


def fused(ctx, S, calls, chg, bal=None, thermal=False, begin=True):
    """The code under test: pack_begin(S), (balance_begin,) charger_begin, then the calls' steps."""
    if begin:
        ctx.pack_begin(S)
        if bal is not None:
            ctx.balance_begin(*bal[:3], compensate=bool(bal[3]))
        ctx.charger_begin(*chg)
    rows = ROWS + (BROWS if bal is not None else ())
    parts = [ctx.step(m, outputs=KEYS, pack=rows, thermal=("temp", "heat") if thermal else None) for m in calls]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["pack"], out["charger"] = ctx.pack_get(), ctx.charger_get()
    if bal is not None:
        out["balance"] = ctx.balance_get()
    return out


def compare(got, ref, what, extra=(), pack_record=True):
    bal = "balance" in got
    for k in KEYS + ROWS + (BROWS if bal else ()) + tuple(extra):
        same(got[k], ref[k], f"{what}: {k}")
    assert tuple(got["charger"]) == cr.FIELDS
    for k in cr.FIELDS:
        same(got["charger"][k], ref["st"]["charger"][k], f"{what}: charger record {k}")
    if pack_record:
        for k in pr.FIELDS:
            same(got["pack"][k], ref["st"]["pack"][k], f"{what}: pack record {k}")
    if bal:
        for k in br.FIELDS:
            same(got["balance"][br.LIB_NAMES[k]], ref["st"]["bal"][k], f"{what}: balance record {k}")


def stats(ref, S, chg):
    """On the reference loop's output: ((string, step) pairs capped by current, by power, pairs
    where an existing current / power cap is loose, pairs whose sequential voltage sum differs from
    the tree's).  At S = 3 the header's tree, (x0 + x1) + x2, is the left-to-right sum itself, so no
    input can tell the two apart there: the sum taken is the right-to-left one, (x2 + x1) + x0."""
    by = ref["capby"]
    im, pm = (np.broadcast_to(np.asarray(a, dtype=np.float64), by.shape[1:]) for a in chg)
    have = by >= 0
    loose_i = int((have & ~np.isnan(im)[None, :] & (by != 1)).sum())
    loose_p = int((have & ~np.isnan(pm)[None, :] & (by != 2)).sum())
    x = np.where(np.isnan(ref["ucmd"]) | np.isnan(ref["vk"]), 0.0, ref["vk"] + 0.0)
    N = x.shape[0]
    x = x.reshape(N, -1, S)
    seq = np.cumsum(x[:, :, ::-1] if S == 3 else x, axis=2)[:, :, -1]   # cumsum adds in index order
    return int((by == 1).sum()), int((by == 2).sum()), loose_i, loose_p, int((seq != ref["vstr"]).sum())


def check_stats(ref, S, chg, what):
    ci, cp, li, lp, order = stats(ref, S, chg)
    print(f"{what}: capped by current in {ci}, by power in {cp} of {ref['capby'].size} (string, step) pairs; loose "
          f"current cap in {li}, loose power cap in {lp}; sequential sum != tree sum in {order}")
    assert ci >= 1 and cp >= 1, "capby = 1 and capby = 2 must both occur"
    assert li >= 1 and lp >= 1, "each cap must be loose somewhere"
    if S >= 3:
        assert order >= 1, "the sequential sum equals the tree sum everywhere: the order would not show"


def pair(M, rom, n, S, nsteps, bal, cfg=None, limits=None, env=None, calls=None, graph=False, soc0=None, tc=None,
         warm=0, chg=None):
    """(reference loop, fused charger) on contexts of one configuration, states included; the caps
    from a cap-free reference loop on a third one unless chg gives them."""
    with _env(**(env or {})):
        a, b, f = M.Context(rom, n, cfg), M.Context(rom, n, cfg), M.Context(rom, n, cfg)
    with a, b, f:
        for c in (a, b, f):
            setup(c, soc0, tc, limits)
            c.step(warm, outputs=())
        if chg is None:
            chg = thresholds(host_loop(f, S, nsteps, NOCAP, bal))
        ref = host_loop(a, S, nsteps, chg, bal)
        b.set_graph(graph)
        got = fused(b, S, calls or (nsteps,), chg, bal)
        ref["state"], got["state"] = a.get_state(), b.get_state()
    return ref, got, chg


def bal_of(par, comp):
    return None if comp is None else tuple(par) + (comp,)


# ---- 1. the host-driven loop equals the fused charger -------------------------------------------
@pytest.mark.parametrize("comp", [None, 0, 1])
@pytest.mark.parametrize("S", sorted(SHAPES))
def test_host_loop_equals_fused_charger(M, rom, S, comp):
    n = S * SHAPES[S]
    assert n <= 2100
    soc0, tc, lim, par = tb.inputs(n, max(S, 2))
    ref, got, chg = pair(M, rom, n, S, NSTEPS, bal_of(par, comp), limits=lim, soc0=soc0, tc=tc)
    check_stats(ref, S, chg, f"S = {S}, compensate = {comp}")
    assert got["vstr"].shape == got["istr"].shape == got["capby"].shape == (NSTEPS, SHAPES[S])
    compare(got, ref, f"S = {S}, compensate = {comp}")
    state_equal(got["state"], ref["state"], f"S = {S}")


# ---- 2. identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nan", "inf", "series_one", "long"])
@pytest.mark.parametrize("balanced", [False, True])
def test_identities(M, rom, case, balanced):
    S = {"series_one": 1, "long": 300}.get(case, 12)
    n, N = 600 if case == "long" else 300, NSTEPS
    soc0, tc, lim, par = tb.inputs(n, max(S, 2))
    chg = (np.inf, np.inf) if case == "inf" else NOCAP
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        for c in (a, b):
            setup(c, soc0, tc, lim)
        a.pack_begin(S)
        if balanced:
            a.balance_begin(*par)
        rows = ("ucmd", "limiter") + (BROWS if balanced else ())
        plain = a.step(N, outputs=KEYS, pack=rows)
        got = fused(b, S, (N,), chg, bal_of(par, 1) if balanced else None)
        for k in KEYS + rows:
            same(got[k], plain[k], f"{case}: {k}")
        for k in pr.FIELDS:
            same(got["pack"][k], a.pack_get()[k], f"{case}: pack record {k}")
        if balanced:
            for k, v in a.balance_get().items():
                same(got["balance"][k], v, f"{case}: balance record {k}")
        state_equal(b.get_state(), a.get_state(), case)
    rec = got["charger"]
    assert (got["capby"] == 0).all() and (rec["ncap_i"] == 0).all() and (rec["ncap_p"] == 0).all()
    assert (rec["steps"] == N).all() and (rec["curtail"] == 0).all() and (rec["nvalid_min"] == S).all()
    x = (plain["v"] + 0.0).reshape(N, -1, S)
    same(got["vstr"], np.stack([[cr.tree_sum(x[t, g]) for g in range(n // S)] for t in range(N)]), f"{case}: vstr")


# ---- 3. NaN cells by construction ---------------------------------------------------------------
@pytest.mark.parametrize("comp", [None, 1])
def test_nan_cells_and_an_all_nan_string(M, rom, comp):
    S, N = 7, 24
    n = 3 * S
    soc0, tc = np.full(n, 30.0), np.full(n, 25.0)
    soc0[:S] = np.linspace(25.0, 40.0, S)
    soc0[S:2 * S] = np.linspace(20.0, 50.0, S)     # string 1: an error cell in the middle
    bad = S + 3
    soc0[bad] = 130.0                              # thetae < 0: in error, its outputs NaN, from its third step on
    soc0[2 * S:] = 130.0                           # string 2: error cells only
    lim = dict(Crate=np.where(np.arange(n) % 2 == 0, 1.0, 2.0))
    par = (np.full(n, 0.25 * tb.I_1C), np.full(n, tb.DZ_ON), np.full(n, tb.DZ_OFF))
    ref, got, chg = pair(M, rom, n, S, N, bal_of(par, comp), limits=lim, soc0=soc0, tc=tc, warm=4,
                         chg=(np.array([20.0, np.nan, 5.0]), np.array([np.nan, 500.0, 50.0])))
    compare(got, ref, "NaN cells")
    state_equal(got["state"], ref["state"], "NaN cells")
    assert got["state"]["status"][bad] & 1 and np.isnan(got["u"][:, bad]).all()
    assert (got["capby"][:, 0] == 1).any() and (got["capby"][:, 1] == 2).any()
    assert (got["charger"]["nvalid_min"] == [S, S - 1, np.nan]).tolist() == [True, True, False]
    assert np.isnan(got["charger"]["nvalid_min"][2]) and got["charger"]["steps"][2] == 0
    assert (got["limiter"][:, 2] == -1).all() and (got["capby"][:, 2] == -1).all() and np.isnan(got["istr"][:, 2]).all()
    assert (got["vstr"][:, 2] == 0).all() and not np.signbit(got["vstr"][:, 2]).any()


# ---- 4. routes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(tb.ROUTES))
def test_routes(M, rom, route):
    n, S, N, kw, percell, env, calls, graph = tb.ROUTES[route]
    N = min(N, NSTEPS)
    if calls:
        calls = {"graph": (6, 6, 6, 6), "calls_7_1_32": (7, 1, 16)}[route]
    soc0, tc, lim, par = tb.inputs(n, S)
    if not percell:   # no set_limits (it would take the route away): the SOC0 spread alone
        lim = None
    ref, got, chg = pair(M, rom, n, S, N, bal_of(par, 1), cfg=M.make_config(**kw), limits=lim, env=env, calls=calls,
                         graph=graph, soc0=soc0, tc=tc)
    ci, cp, *_ = stats(ref, S, chg)
    print(f"{route}: capped by current in {ci}, by power in {cp}")
    assert ci >= 1 and cp >= 1
    compare(got, ref, route)
    state_equal(got["state"], ref["state"], route)


def test_routes_without_a_balancer_graph_and_calls(M, rom):
    n, S = 240, 12
    soc0, tc, lim, _ = tb.inputs(n, S)
    ref, got, chg = pair(M, rom, n, S, 24, None, limits=lim, calls=(6, 6, 6, 5, 1), graph=True, soc0=soc0, tc=tc)
    check_stats(ref, S, chg, "graph, no balancer")
    compare(got, ref, "graph, no balancer")
    state_equal(got["state"], ref["state"], "graph, no balancer")


# ---- 5. with the other pack features ------------------------------------------------------------
@pytest.mark.parametrize("links", [False, True])
def test_thermal_model_schedule_and_links(M, rom, links):
    n, S, N = 192, 16, NSTEPS
    soc0, _, _, par = tb.inputs(n, S)
    p, th, sched, rng = tb._thermal(M, rom, n)
    bal = bal_of(par, 1)
    r_link = rng.uniform(0.5, 3.0, n)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as f:
        for c in (a, b, f):
            setup(c, soc0, p["T0"], None, th, sched)
        for c in (a, f) if links else ():              # links need strings: the reference is a charger-free pack
            c.pack_begin(S)
            c.thermal_couple(r_link)
        chg = thresholds(host_loop(f, S, N, NOCAP, bal, thermal=True, packed=links))
        ref = host_loop(a, S, N, chg, bal, thermal=True, packed=links)
        b.pack_begin(S)
        if links:
            b.thermal_couple(r_link)
        b.balance_begin(*par)
        b.charger_begin(*chg)
        got = fused(b, S, (N,), chg, bal, thermal=True, begin=False)
        compare(got, ref, "thermal", extra=("temp", "heat"), pack_record=not links)   # a's own pack counted its own reduction
        if links:
            for k, v in a.thermal_couple_get().items():
                same(b.thermal_couple_get()[k], v, f"links: couple record {k}")
        for k, v in a.thermal_get().items():
            same(b.thermal_get()[k], v, f"thermal record {k}")
        state_equal(b.get_state(), a.get_state(), "thermal")
    ci, cp, *_ = stats(ref, S, chg)
    assert ci >= 1 and cp >= 1


def test_step_summary(M, rom):
    n, S, N = 240, 12, 70                               # 70 steps: a full 64-row window and a partial one
    soc0, tc, lim, par = tb.inputs(n, S)
    bal = bal_of(par, 1)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as f:
        for c in (a, b, f):
            setup(c, soc0, tc, lim)
        chg = thresholds(host_loop(f, S, NSTEPS, NOCAP, bal))
        ref = host_loop(a, S, N, chg, bal)
        b.pack_begin(S)
        b.balance_begin(*par)
        b.charger_begin(*chg)
        b.summary_begin()
        b.step_summary(30)
        b.step_summary(40)
        got = b.get_summary()
        sr.same_record(got, sr.reduce(ref), "summary", fields=[k for k in sr.FIELDS if not k.startswith("obs_")])
        rec = dict(charger=b.charger_get(), pack=b.pack_get(), balance=b.balance_get())
        for k in cr.FIELDS:
            same(rec["charger"][k], ref["st"]["charger"][k], f"summary: charger record {k}")
        for k in pr.FIELDS:
            same(rec["pack"][k], ref["st"]["pack"][k], f"summary: pack record {k}")
        for k in br.FIELDS:
            same(rec["balance"][br.LIB_NAMES[k]], ref["st"]["bal"][k], f"summary: balance record {k}")
        state_equal(b.get_state(), a.get_state(), "summary")
    same(got["u_last"], ref["u"][-1], "u_last is the cell's own applied current")
    assert (ref["capby"] > 0).any()


def test_aging_estimate_source(M, rom):
    import test_gpu_aging as ta
    n, S, N = 240, 12, NSTEPS
    soc0, tc, lim, par = tb.inputs(n, S)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as f:
        for c in (a, b, f):
            setup(c, soc0, tc, lim)
            c.aging_begin(ta.reactions(n, 2), sources=("est",))
        chg = thresholds(host_loop(f, S, N, NOCAP))
        ref = host_loop(a, S, N, chg)
        got = fused(b, S, (N,), chg)
        compare(got, ref, "aging")
        tb._same_tree(b.aging_record(), a.aging_record(), "aging record")
        state_equal(b.get_state(), a.get_state(), "aging")
    assert (ref["capby"] > 0).any()


def test_termination_and_step_until(M, rom):
    """A latched cell's string rests at 0 A and is never capped; step_until runs on NULL outputs,
    so k_term and k_charger read the context's own soc row."""
    n, S, N = 240, 12, NSTEPS
    soc0, tc, lim, par = tb.inputs(n, S)
    bal = bal_of(par, 1)
    top = soc0.reshape(-1, S).argmax(axis=1) + S * np.arange(n // S)
    soc_stop = np.full(n, 2.0)
    soc_stop[top] = soc0[top] / 100.0 + 0.02
    soc_stop[top[::3]] = 2.0
    stop = dict(soc_stop=soc_stop)
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as c3, M.Context(rom, n) as f:
        for c in (a, b, c3, f):
            setup(c, soc0, tc, lim)
        chg = thresholds(host_loop(f, S, N, NOCAP, bal, stop=stop, T=tc))
        ref = host_loop(a, S, N, chg, bal, stop=stop, T=tc)
        for c in (b, c3):
            c.pack_begin(S)
            c.balance_begin(*par)
            c.charger_begin(*chg)
            c.term_begin(**stop)
        got = fused(b, S, (7, 1, 16), chg, bal, begin=False)
        rest = ref["mraw"] == 0
        assert rest.any() and (ref["capby"][rest] == 0).all() and (ref["capby"] > 0).any()
        compare(got, ref, "termination")
        for k in tr.FIELDS:
            same(b.term_get()[k], tr.record(ref["tst"])[k], f"termination: term record {k}")
        state_equal(b.get_state(), a.get_state(), "termination")
        run, left = c3.step_until(N, chunk=8)
        assert run == N and left == int((ref["tst"]["state"] == tr.OPEN).sum())
        for k in cr.FIELDS:
            same(c3.charger_get()[k], ref["st"]["charger"][k], f"step_until: charger record {k}")
        state_equal(c3.get_state(), a.get_state(), "step_until")


# ---- 6. begin -> end -> begin, refusals, the wrappers -------------------------------------------
def test_begin_steps_end_steps_begin(M, rom):
    n, S = 240, 12
    soc0, tc, lim, par = tb.inputs(n, S)
    chg = (np.full(n // S, 20.0), np.full(n // S, 700.0))
    with M.Context(rom, n) as a, M.Context(rom, n) as b, M.Context(rom, n) as twin:
        for c in (a, b, twin):
            setup(c, soc0, tc, lim)
        ref = host_loop(a, S, 10, chg)
        b.set_graph(True)
        got = fused(b, S, (5, 5), chg)
        compare(got, ref, "before the end")
        assert (got["capby"] > 0).any()
        b.charger_end()
        b.charger_end()                                # a no-op without a begin
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: charger_get"):
            b.charger_get()
        twin.set_state(b.get_state())                  # a charger-free pack started from that state
        twin.pack_begin(S)
        x, y = b.step(5, outputs=KEYS, pack=("ucmd", "limiter")), twin.step(5, outputs=KEYS, pack=("ucmd", "limiter"))
        for k in x:
            same(x[k], y[k], f"after the end: {k}")
        state_equal(b.get_state(), twin.get_state(), "after the end")
        a.set_state(b.get_state())                     # begin again: the record starts over
        ref = host_loop(a, S, 5, chg)
        b.charger_begin(*chg)
        o = b.step(5, outputs=KEYS, pack=ROWS)
        for k in KEYS + ROWS:
            same(o[k], ref[k], f"after the second begin: {k}")
        for k in cr.FIELDS:
            same(b.charger_get()[k], ref["st"]["charger"][k], f"after the second begin: charger record {k}")
        b.pack_end()                                   # pack_end ends a charger too
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: charger_get"):
            b.charger_get()
        # pack_begin with the same S keeps the charger, with another S ends it: its arrays are per string
        b.pack_begin(S)
        b.charger_begin(*chg)
        b.step(3, outputs=())
        b.pack_begin(S)
        assert (b.charger_get()["steps"] == 3).all()
        b.pack_begin(S // 2)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: charger_get"):
            b.charger_get()
        b.charger_begin(i_max=20.0)                    # scalars, before ...
        assert b.charger_get()["steps"].shape == (2 * n // S,)
    with M.Context(rom, n) as c:                       # ... and before init_cells
        c.pack_begin(S)
        c.charger_begin(p_max=700.0)
        setup(c, soc0, tc, lim)
        assert (c.step(3, pack=("capby",))["capby"] >= 0).all()


def test_refusals_change_nothing(M, rom):
    n, S = 36, 12
    soc0, tc, lim, par = tb.inputs(n, S)
    chg = (np.full(3, 20.0), np.full(3, 700.0))
    with M.Context(rom, n) as ctx:
        setup(ctx, soc0, tc, lim)
        ctx.step(3, outputs=())
        st0 = ctx.get_state()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: charger_begin: call mpcekf_pack_begin first"):
            ctx.charger_begin(20.0, 700.0)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: charger_get"):
            ctx.charger_get()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_charger: call mpcekf_charger_begin first"):
            ctx.step(2, pack=ROWS)
        state_equal(ctx.get_state(), st0, "refused without a pack")
        ctx.pack_begin(S)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_charger: call mpcekf_charger_begin first"):
            ctx.step(2, pack=("vstr",))
        state_equal(ctx.get_state(), st0, "refused without a charger")
        assert (ctx.pack_get()["steps"] == 0).all()
        ctx.charger_begin(*chg)
        ctx.step(5, outputs=())
        st1, rec1, pk1 = ctx.get_state(), ctx.charger_get(), ctx.pack_get()
        assert (rec1["steps"] == 5).all() and rec1["ncap_i"].sum() + rec1["ncap_p"].sum() > 0
        L, lib = ctx.L, M._lib
        for row, v, msg in ((0, -0.1, "i_max"), (0, -np.inf, "i_max"), (1, 0.0, "p_max"), (1, -3.0, "p_max")):
            p = np.ascontiguousarray(np.stack(chg))
            p[row, 2] = v
            assert L.mpcekf_charger_begin(ctx.h, lib.dptr(p)) == -1 and msg.encode() in L.mpcekf_last_error()
        assert L.mpcekf_charger_begin(ctx.h, None) == -1
        ids, vals = np.array([0, 0], dtype=np.int32), np.full((2, 3), 7.0)
        assert L.mpcekf_charger_get(ctx.h, 2, lib.iptr(ids), lib.dptr(vals)) == -1     # a repeated id
        assert L.mpcekf_charger_get(ctx.h, 10, lib.iptr(ids), lib.dptr(vals)) == -1
        ids[1] = 9
        assert L.mpcekf_charger_get(ctx.h, 2, lib.iptr(ids), lib.dptr(vals)) == -1 and (vals == 7.0).all()
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_charger: bleed / zmin rows"):
            ctx.step(2, pack=("vstr", "bleed"))
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_ex_charger: temp / heat rows"):
            ctx.step(2, pack=("vstr",), thermal=("temp",))
        state_equal(ctx.get_state(), st1, "refused with a charger")
        for k in rec1:
            same(ctx.charger_get()[k], rec1[k], f"refused with a charger: charger record {k}")
        for k in pk1:
            same(ctx.pack_get()[k], pk1[k], f"refused with a charger: pack record {k}")
        ctx.charger_begin(*chg)                            # a second begin replaces the first, record reset
        rec = ctx.charger_get()
        assert all((rec[k] == 0).all() for k in cr.FIELDS[:6]) and all(np.isnan(rec[k]).all() for k in cr.FIELDS[6:])


def test_wrappers_pass_the_charger_through(M, rom):
    n, S, N = 36, 12, 12
    soc0, tc, lim, par = tb.inputs(n, S)
    bal = dict(i_bleed=par[0], dz_on=tb.DZ_ON, dz_off=tb.DZ_OFF, compensate=True)
    chg = dict(i_max=np.array([20.0, np.nan, 40.0]), p_max=np.array([np.nan, 700.0, 600.0]))
    out = M.runMPC(rom, soc0, tc, N, limits=lim, pack=dict(series=S, balance=bal, charger=chg))
    # the rule on the run's own ucmd / soc rows; the voltages from the string voltages it reports
    assert out["vstr"].shape == (N, 3) and (out["capby"] > 0).any()
    x = (out["v"] + 0.0).reshape(N, -1, S)
    same(out["vstr"], np.stack([[cr.tree_sum(x[t, g]) for g in range(3)] for t in range(N)]), "runMPC: vstr")
    r = cr.step(out["ucmd"], out["soc"], out["v"], S, chg["i_max"], chg["p_max"], balance=tuple(par) + (1,))
    for k in ("u", "limiter", "istr", "capby", "bleed", "zmin"):
        same(out[k], r[k], f"runMPC: {k}")
    s = M.run_summary(rom, soc0, tc, N, limits=lim, pack=dict(series=S, balance=bal, charger=chg), chunk=5)
    for k in cr.FIELDS:
        same(out["charger"][k], r["st"]["charger"][k], f"runMPC: charger record {k}")
        same(s["charger"][k], r["st"]["charger"][k], f"run_summary: charger record {k}")
    same(s["u_last"], out["u"][-1], "run_summary: u_last")
