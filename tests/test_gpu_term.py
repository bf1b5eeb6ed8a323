"""GPU: charge termination along the fused loop (mpcekf_term_begin / _get / _open / _end,
mpcekf_step_until; k_term after Hildreth, before k_pack, in every fused step).

The reference everywhere is the host-driven loop the feature replaces, on a second context that
has no termination rule: per step, step(1), get_state, tests/term_ref.py (the header's rule in
plain numpy) on the step's soc row, the uk column and the temperature the step used (then, on a
pack, tests/pack_ref.py on the result), uk / uk_1 written back with set_state({"scal": ...}).
Every comparison is bitwise (a NaN equals a NaN).  Nothing expected comes from the code under
test.  The thresholds are chosen on the CPU from a C-oracle run of the same inputs: soc_stop
half-way between the oracle's SOC at two consecutive steps, the later one a step drawn from 5..28
per cell (soc0 / 100 + delta; on the tests' synthetic ROM the SOC estimate rises about 0.4 % in a
2 C step, not the 0.055 % of the full-size cell, so delta runs over 1..8 % of SOC where the
full-size cell's would over 0.2..1.5 %), a group below soc0 (latched at step 1) and a group out
of reach; i_taper from the oracle's own current under a low v_max.  Every case asserts on the
reference, before it compares, that cells latch at step 1, in steps 5..30, and never.

  1. a plain context: each criterion alone and all together, hold 1 and 3
  2. packs, S in {1, 2, 5, 100, 200}
  3. routes
  4. identity: thresholds that never hold; after term_end
  5. step_until
  6. two runs of a pack case give the same bits
  7. refusals
"""
import contextlib
import os

import numpy as np
import pytest

import pack_ref as pr
import summary_ref as sr
import term_ref as tr

pytestmark = pytest.mark.gpu

KEYS = ("u", "v", "soc", "phise", "nexec")
S_UK_1, S_UK = 5, 6          # MPCEKF_S_UK_1, MPCEKF_S_UK
N, NSTEPS, CALLS = 200, 40, (7, 1, 32)   # three full waves and a ragged one; window, graph-shape and parity changes


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


def inputs(n, seed=0x7E23):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(10.0, 60.0, n), np.full(n, 25.0), rng


def spread(base, rng, lo, hi, below, far):
    """Per-cell thresholds: base + delta with delta over lo..hi (latching inside the run); the
    cells 1 mod 6 at base - below (latched at step 1), the cells 4 mod 6 at base + far (out of
    reach)."""
    n = base.shape[0]
    th = base + rng.uniform(lo, hi, n)
    i = np.arange(n)
    th[i % 6 == 1] = base[i % 6 == 1] - below
    th[i % 6 == 4] = base[i % 6 == 4] + far
    return th


_ORACLE = {}


def soc_stop(oc, rom, soc0, tc, rng, nsteps=NSTEPS, early=None, never=None, last=28):
    """soc_stop per cell from the C oracle's run of the same inputs (default configuration): half-way
    between its SOC at two consecutive steps, the later one step j (1-based) drawn from 5..last, so
    the cell latches at step j where the run under test follows the oracle; the cells of `early`
    (default 1 mod 6) 1 % under soc0: latched at step 1; the cells of `never` (default 4 mod 6) out
    of reach."""
    key = (soc0.tobytes(), tc.tobytes(), nsteps)
    if key not in _ORACLE:
        _ORACLE[key] = oc.run(rom, soc0, tc, nsteps)["soc"]
    soc, n = _ORACLE[key], soc0.shape[0]
    i = np.arange(n)
    j = rng.integers(5, min(last, nsteps - 1) + 1, n)
    th = 0.5 * (soc[j - 2, i] + soc[j - 1, i])
    early = i % 6 == 1 if early is None else early
    never = i % 6 == 4 if never is None else never
    th[early] = soc0[early] / 100.0 - 0.01
    th[never] = 2.0
    return th


def groups(rec, nsteps, what, need=("first", "mid", "never")):
    """On the reference's record: cells latched at step 1, in steps 5..30 (roughly a third of them
    in a 40-step run: a quarter is asked for), and never.  need: the groups the case can have (the
    taper needs a step to arm: none at step 1; one string of every cell has one fate)."""
    d, s = rec["done_step"], rec["state"]
    got = dict(first=int(((d == 1) & (s == 1)).sum()), mid=int(((d >= 5) & (d <= 30) & (s == 1)).sum()),
               never=int((s == 0).sum()))
    print(f"{what}: latched at step 1: {got['first']}, in steps 5..30: {got['mid']}, never: {got['never']} of {d.size}; "
          f"reasons {sorted(set(rec['reason'].astype(int).tolist()))}")
    for k in need:
        assert got[k] >= (d.size // 4 if k == "mid" and nsteps >= 40 else 1), (what, k, got)


def host_loop(ctx, nsteps, stop, T=None, S=None, thermal=False, packed=False, st=None, rec=None):
    """The reference: nsteps times step(1) + get_state + term_ref (+ pack_ref) + set_state on a
    context without a rule.  T: the cells' temperature when no model sets it.  packed: the context
    is a pack itself (for the links): the cells' own commands are its ucmd row.  Returns the
    per-step rows, the record, the open count after every step."""
    n = ctx.n
    st = tr.reset(n) if st is None else st
    th = ("temp", "heat") if thermal else None
    rows = {k: [] for k in KEYS + (("ucmd", "limiter") if S else ()) + (th or ())}
    opens = []
    for _ in range(nsteps):
        o = ctx.step(1, outputs=KEYS, thermal=th, pack=("ucmd",) if packed else None)
        scal = ctx.get_state()["scal"]
        own = o["ucmd"][0].copy() if packed else scal[:, S_UK].copy()
        u, st = tr.step(st, o["soc"][0], own, o["temp"][0] if thermal else T, series=S, **stop)
        rest = (st["state"] == tr.LATCHED) & ~np.isnan(own)
        if packed:                                   # k_pack of the rule-free context has been there: put the own commands back
            ok = ~np.isnan(own)
            scal[ok, S_UK] = own[ok]
        scal[rest, S_UK] = 0.0
        scal[rest, S_UK_1] = 0.0
        if S:
            r = pr.reduce(u[None, :], S, state=rec)
            rec = {k: r[k] for k in pr.FIELDS}
            ok = ~np.isnan(u)
            scal[ok, S_UK] = r["u"][0][ok]
            scal[ok, S_UK_1] = r["u"][0][ok]
            rows["ucmd"].append(u)
            rows["limiter"].append(r["limiter"][0])
            u = r["u"][0]
        ctx.set_state({"scal": scal})
        for k in KEYS[1:] + (th or ()):
            rows[k].append(o[k][0])
        rows["u"].append(u)
        opens.append(tr.n_open(st))
    out = {k: np.stack(v) for k, v in rows.items()}
    out["term"], out["st"], out["opens"], out["pack"] = tr.record(st), st, opens, rec
    return out


def fused(ctx, calls, stop, S=None, thermal=False):
    """The code under test: (pack_begin,) term_begin, then the calls' steps, rows concatenated."""
    if S:
        ctx.pack_begin(S)
    ctx.term_begin(**stop)
    parts = [ctx.step(m, outputs=KEYS, thermal=("temp", "heat") if thermal else None,
                      pack=("ucmd", "limiter") if S else None) for m in calls]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["term"] = ctx.term_get()
    out["open"] = ctx.term_open()
    if S:
        out["pack"] = ctx.pack_get()
    return out


def compare(got, ref, what, extra=()):
    for k in KEYS + tuple(extra):
        same(got[k], ref[k], f"{what}: {k}")
    assert tuple(got["term"]) == tr.FIELDS
    for k in tr.FIELDS:
        same(got["term"][k], ref["term"][k], f"{what}: term record {k}")
    assert got["open"] == ref["opens"][-1], what
    if "state" in ref:
        state_equal(got["state"], ref["state"], what)


def setup(ctx, soc0, tc, limits=None, thermal=None, schedule=None):
    ctx.init_cells(soc0, tc)
    if limits:
        ctx.set_limits(**limits)
    if thermal:
        ctx.thermal_begin(**thermal)
    if schedule:
        ctx.thermal_schedule(*schedule[0], **schedule[1])


def pair(M, rom, n, nsteps, stop, calls=None, cfg=None, limits=None, env=None, graph=None, soc0=None, tc=None, S=None,
         thermal=None, schedule=None, links=None, aging=None, what="", need=("first", "mid", "never")):
    """(reference loop, fused run) on two contexts of one configuration, states and the other
    records included; the groups are asserted on the reference before anything is compared."""
    with _env(**(env or {})):
        a, b = M.Context(rom, n, cfg), M.Context(rom, n, cfg)
    with a, b:
        for c in (a, b):
            setup(c, soc0, tc, limits, thermal, schedule)
            if aging:
                c.aging_begin(aging, sources=("est", "plant"))
        if links is not None:                       # links need strings: the reference is a pack without a rule
            a.pack_begin(S)
            a.thermal_couple(links)
        ref = host_loop(a, nsteps, stop, T=tc, S=S, thermal=bool(thermal), packed=links is not None)
        groups(ref["term"], nsteps, what, need)
        if graph is not None:
            b.set_graph(graph)
        if links is not None:
            b.pack_begin(S)
            b.thermal_couple(links)
        got = fused(b, calls or (nsteps,), stop, S=S, thermal=bool(thermal))
        ref["state"], got["state"] = a.get_state(), b.get_state()
        for name, get in (("thermal", "thermal_get"), ("aging", "aging_record"), ("couple", "thermal_couple_get")):
            if {"thermal": thermal, "aging": aging, "couple": links}[name] is not None:
                ref[name], got[name] = getattr(a, get)(), getattr(b, get)()
    return ref, got


def records_equal(got, ref, names, what):
    """The other records of the two contexts: {field: [n]}, or aging_record's {source: [{field: [n]}]}."""
    for name in names:
        ra, rb = ref[name], got[name]
        if name == "aging":
            ra, rb = ({f"{s}.{i}.{k}": v for s, rs in r.items() for i, d in enumerate(rs) for k, v in d.items()} for r in (ra, rb))
        assert set(ra) == set(rb) and ra, (what, name)
        for k in ra:
            same(rb[k], ra[k], f"{what}: {name} record {k}")


_TAPER = {}


def taper_latch(au, it, hold):
    """The 1-based step at which the header's taper counter fires on the current magnitudes au, 0: never."""
    armed, run = False, 0
    for t, x in enumerate(au, 1):
        if x > it:
            armed, run = True, 0
        elif armed:
            run += 1
        else:
            run = 0
        if run >= hold:
            return t
    return 0


def taper_case(oc, rom, hold):
    """Inputs whose current tapers within the run, from the C oracle on the CPU: SOC0 on eight
    levels and, per cell, a v_max 20, 30 or 40 mV (the cells in turn) under the voltage the oracle's
    unlimited 2 C charge of that cell reaches at its seventh step, so the voltage row binds within
    some ten steps.  The oracle's current then falls in a zig-zag (every other step back near the
    2 C bound), which breaks runs of small currents by itself.  i_taper per cell: among the
    half-way points between neighbouring values of the oracle's own sorted |u| that lie 5 mA or more
    from both, one at which the header's counter, run over the oracle's |u| with this hold, fires
    in steps 5..30, drawn at random; for the cells 4 mod 6 a quarter of the smallest current of the
    run: never reached.  The oracle takes one v_max per run, so it runs once per (level, v_max)
    pair, 24 times.  -> (soc0, tc, limits, i_taper)"""
    if hold not in _TAPER:
        rng = np.random.Generator(np.random.PCG64(0x7A9E))
        level = rng.integers(0, 8, N)
        soc0, tc, i = np.linspace(12.0, 58.0, 8)[level], np.full(N, 25.0), np.arange(N)
        free = oc.run(rom, np.linspace(12.0, 58.0, 8), np.full(8, 25.0), 12)
        v_max, it, planned = np.empty(N), np.empty(N), np.zeros(N, dtype=int)
        for lv in range(8):
            for g in range(3):
                m = np.flatnonzero((level == lv) & (i % 3 == g))
                if not m.size:
                    continue
                vm = float(free["v"][6, lv]) - 0.02 - 0.01 * g
                au = np.abs(oc.run(rom, soc0[m[:1]], tc[:1], NSTEPS, v_max=vm)["u"][:, 0])
                vals = np.unique(au)
                cand = [(0.5 * (a + b), taper_latch(au, 0.5 * (a + b), hold)) for a, b in zip(vals[:-1], vals[1:]) if b - a >= 0.01]
                cand = [(x, t) for x, t in cand if 5 <= t <= 30]
                assert cand, f"the oracle's current does not taper at SOC0 {soc0[m[0]]:.0f} %, v_max {vm:.3f} V"
                v_max[m] = vm
                pick = rng.integers(0, len(cand), m.size)
                it[m] = [cand[k][0] for k in pick]
                planned[m] = [cand[k][1] for k in pick]
                off = m[m % 6 == 4]
                it[off], planned[off] = 0.25 * au.min(), 0
        print(f"taper, hold {hold}: planned latch steps on the oracle's current: {np.bincount(planned)[1:].tolist()} (steps 1..), "
              f"never: {int((planned == 0).sum())}")
        _TAPER[hold] = dict(soc0=soc0, tc=tc, limits=dict(v_max=v_max), it=it)
    T = _TAPER[hold]
    return T["soc0"], T["tc"], T["limits"], T["it"].copy()


def thermal_params(n):
    import test_gpu_thermal as tg
    p = tg.params(n)
    rng = np.random.Generator(np.random.PCG64(0x7C07))
    p["soc0"] = rng.uniform(10.0, 60.0, n)
    p["Cth"] = rng.uniform(20.0, 60.0, n)              # J/K: kelvins within the run
    return p, rng


# ---- 1. a plain context -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["soc", "taper_hold1", "taper_hold3", "T_cut", "all_hold1", "all_hold3"])
def test_plain_context(M, rom, oc, case):
    soc0, tc, rng = inputs(N)
    stop, limits, thermal, i = {}, None, None, np.arange(N)
    if case.startswith(("taper", "all")):
        soc0, tc, limits, it = taper_case(oc, rom, int(case[-1]))
        stop.update(i_taper=it, hold=int(case[-1]))
    if case in ("soc",) or case.startswith("all"):
        th = soc_stop(oc, rom, soc0, tc, rng)
        if case.startswith("all"):   # the sixes of cells in turn: the SOC, the taper, the temperature first; the early cells by SOC
            th[(i // 6 % 3 != 0) & (i % 6 != 1)] = 2.0
            stop["i_taper"] = np.where(i // 6 % 3 == 1, stop["i_taper"], np.nan)
        stop["soc_stop"] = th
    if case == "T_cut" or case.startswith("all"):
        p, prng = thermal_params(N)
        if case == "T_cut":
            soc0, tc = p["soc0"], p["T0"]
        thermal = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom))
        cut = spread(tc.copy(), prng, 0.05, 0.8, 1.0, 50.0)
        if case.startswith("all"):
            cut[i // 6 % 3 != 2] = 90.0
        stop["T_cut"] = cut
    need = ("mid", "never") if case.startswith("taper") else ("first", "mid", "never")
    ref, got = pair(M, rom, N, NSTEPS, stop, calls=CALLS, limits=limits, soc0=soc0, tc=tc, thermal=thermal, what=case,
                    need=need)
    want = {"soc": {0, 1}, "T_cut": {0, 4}}.get(case, {0, 2} if case.startswith("taper") else {0, 1, 2, 4})
    assert want <= set(ref["term"]["reason"].astype(int).tolist()), (case, want)
    compare(got, ref, case, extra=("temp", "heat") if thermal else ())
    if thermal:
        records_equal(got, ref, ("thermal",), case)


# ---- 2. packs -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def no_pack(M, rom, oc):
    soc0, tc, rng = inputs(N)
    stop = dict(soc_stop=soc_stop(oc, rom, soc0, tc, rng))
    with M.Context(rom, N) as b:
        setup(b, soc0, tc)
        got = fused(b, CALLS, stop)
        got["state"] = b.get_state()
    return got


def pack_thresholds(oc, rom, S, soc0, tc, rng, nsteps=NSTEPS):
    """soc_stop for strings of S: a string stops with its first cell, so the cells latched at step
    1 stay in string 0 (where there are three strings or more; none otherwise), the last fifth of
    the strings (the second of two) is out of reach, and the others latch inside the run.
    -> (thresholds, the groups the reference can have)."""
    if S == 1:
        return soc_stop(oc, rom, soc0, tc, rng, nsteps), ("first", "mid", "never")
    n = soc0.shape[0]
    g, nstr = np.arange(n) // S, n // S
    early = (np.arange(n) % 6 == 1) & (g == 0) & (nstr >= 3)
    never = (g >= nstr - max(1, nstr // 5)) & (nstr >= 2)
    th = soc_stop(oc, rom, soc0, tc, rng, nsteps, early=early, never=never)
    return th, ("first", "mid", "never") if nstr >= 3 else ("never",) if nstr == 2 else ()


@pytest.mark.parametrize("S", [1, 2, 5, 100, 200])
def test_packs(M, rom, oc, no_pack, S):
    soc0, tc, rng = inputs(N)
    th, need = pack_thresholds(oc, rom, S, soc0, tc, rng)
    stop = dict(soc_stop=th)
    ref, got = pair(M, rom, N, NSTEPS, stop, calls=CALLS, soc0=soc0, tc=tc, S=S, what=f"S = {S}", need=need)
    d = ref["term"]
    if S > 1:
        lagged = d["reason"] == 8
        assert lagged.any(), "no cell followed its string"
        first = d["done_step"].reshape(-1, S).copy()
        first[d["reason"].reshape(-1, S) == 8] = np.inf
        first[first == 0] = np.inf
        lag = d["done_step"].reshape(-1, S) - first.min(axis=1, keepdims=True)
        assert (lag[d["reason"].reshape(-1, S) == 8] == 1).all(), "string-mates follow exactly one step late"
    compare(got, ref, f"S = {S}")
    for k in ("ucmd", "limiter"):
        same(got[k], ref[k], f"S = {S}: {k}")
    for k in pr.FIELDS:
        same(got["pack"][k], ref["pack"][k], f"S = {S}: pack record {k}")
    if S == 1:   # the same thresholds on a context without a pack
        for k in KEYS:
            same(got[k], no_pack[k], f"S = 1 vs no pack: {k}")
        for k in tr.FIELDS:
            same(got["term"][k], no_pack["term"][k], f"S = 1 vs no pack: term record {k}")
        state_equal(got["state"], no_pack["state"], "S = 1 vs no pack")


# ---- 3. routes ----------------------------------------------------------------------------------
ROUTES = {
    # name: (n, N, make_config keywords, per-cell limits?, environment, calls, graph, S)
    "mask_eta_off": (N, NSTEPS, dict(constraints=(1, 1, 0)), False, {}, CALLS, None, None),
    "percell": (N, NSTEPS, {}, True, {}, CALLS, None, None),
    "mb": (N, NSTEPS, dict(method="MB"), False, {}, CALLS, None, None),
    "np20": (24, 12, dict(Np=20, Nc=10), False, {}, (7, 1, 4), None, None),
    "split_cell": (N, NSTEPS, {}, False, dict(MPCEKF_QUAD=0, MPCEKF_SPLIT_CELL=1), CALLS, None, None),
    # a repeated call shape replays one graph: the string flags' parity is the call's own (strings of 5)
    "graph_on": (N, NSTEPS, {}, False, {}, (7, 1, 8, 8, 8, 8), True, 5),
    "graph_off": (N, NSTEPS, {}, False, {}, (7, 1, 8, 8, 8, 8), False, 5),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(M, rom, oc, route):
    n, nsteps, kw, percell, env, calls, graph, S = ROUTES[route]
    soc0, tc, rng = inputs(n)
    th, need = pack_thresholds(oc, rom, S or 1, soc0, tc, rng, nsteps)
    limits = dict(Crate=np.where(np.arange(n) % 2 == 0, 2.0, 1.5)) if percell else None
    ref, got = pair(M, rom, n, nsteps, dict(soc_stop=th), calls=calls, cfg=M.make_config(**kw), limits=limits, env=env,
                    graph=graph, soc0=soc0, tc=tc, S=S, what=route, need=need)
    compare(got, ref, route)
    if S:
        assert (ref["term"]["reason"] == 8).any()
        for k in ("ucmd", "limiter"):
            same(got[k], ref[k], f"{route}: {k}")


def test_step_summary(M, rom, oc):
    soc0, tc, rng = inputs(N)
    stop = dict(soc_stop=soc_stop(oc, rom, soc0, tc, rng))
    with M.Context(rom, N) as a, M.Context(rom, N) as b:
        for c in (a, b):
            setup(c, soc0, tc)
        ref = host_loop(a, NSTEPS, stop, T=tc)
        groups(ref["term"], NSTEPS, "summary")
        b.summary_begin(reach=0.5)
        b.term_begin(**stop)
        for m in CALLS:
            b.step_summary(m)
        got = b.get_summary()
        sr.same_record(got, sr.reduce(ref, reach=0.5), "summary", fields=[k for k in sr.FIELDS if not k.startswith("obs_")])
        for k in tr.FIELDS:
            same(b.term_get()[k], ref["term"][k], f"summary: term record {k}")
        state_equal(b.get_state(), a.get_state(), "summary")
    same(got["u_last"], ref["u"][-1], "u_last is the resting current")


def test_thermal_model_and_schedule(M, rom, oc):
    p, rng = thermal_params(N)
    th = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom))
    grid = np.linspace(0.0, 1.0, 5)
    sched = ((20.0, 40.0), dict(sets=(np.arange(N) % 3).astype(np.int32),
                                Crate=np.stack([2.0 - 0.8 * grid, 1.6 - 0.5 * grid, 1.2 - 0.3 * grid])))
    stop = dict(soc_stop=soc_stop(oc, rom, p["soc0"], p["T0"], rng),
                T_cut=np.where(np.arange(N) % 2 == 0, p["T0"] + rng.uniform(0.05, 0.8, N), np.nan))
    ref, got = pair(M, rom, N, NSTEPS, stop, calls=CALLS, soc0=p["soc0"], tc=p["T0"], thermal=th, schedule=sched,
                    what="thermal + schedule")
    compare(got, ref, "thermal + schedule", extra=("temp", "heat"))
    records_equal(got, ref, ("thermal",), "thermal + schedule")


def test_conduction_links(M, rom, oc):
    n, S = 192, 12
    p, rng = thermal_params(n)
    th = dict(Cth=p["Cth"], Rth=p["Rth"], Tamb=p["Tamb"], ocv=M.thermal_ocv(rom))
    links = rng.uniform(0.5, 3.0, n)
    # no cell latched at step 1, and the last three strings never stop
    soc = soc_stop(oc, rom, p["soc0"], p["T0"], rng, early=np.zeros(n, dtype=bool), never=np.arange(n) >= n - 3 * S)
    ref, got = pair(M, rom, n, NSTEPS, dict(soc_stop=soc), calls=CALLS, soc0=p["soc0"], tc=p["T0"], thermal=th, S=S,
                    links=links, what="links", need=("mid", "never"))
    compare(got, ref, "links", extra=("temp", "heat"))
    for k in ("ucmd", "limiter"):
        same(got[k], ref[k], f"links: {k}")
    records_equal(got, ref, ("thermal", "couple"), "links")


def test_aging(M, rom, oc):
    import test_gpu_aging as ta
    soc0, tc, rng = inputs(N)
    stop = dict(soc_stop=soc_stop(oc, rom, soc0, tc, rng))
    ref, got = pair(M, rom, N, NSTEPS, stop, calls=CALLS, soc0=soc0, tc=tc, aging=ta.reactions(N, 2), what="aging")
    compare(got, ref, "aging")
    records_equal(got, ref, ("aging",), "aging")


# ---- 4. identity --------------------------------------------------------------------------------
@pytest.mark.parametrize("never", ["nan", "finite"])
def test_thresholds_that_never_hold_are_the_identity(M, rom, never):
    soc0, tc, _ = inputs(N)
    stop = {} if never == "nan" else dict(soc_stop=2.0, i_taper=-1.0, hold=1, T_cut=1000.0)
    with M.Context(rom, N) as a, M.Context(rom, N) as b:
        for c in (a, b):
            setup(c, soc0, tc)
        b.term_begin(**stop)
        for m in CALLS:
            x, y = a.step(m, outputs=KEYS), b.step(m, outputs=KEYS)
            for k in KEYS:
                same(y[k], x[k], f"{never}: {k}")
        state_equal(b.get_state(), a.get_state(), never)
        rec = b.term_get()
        assert b.term_open() == N and (rec["state"] == 0).all() and (rec["steps"] == NSTEPS).all() and (rec["rest"] == 0).all()
        b.term_end()
        b.term_end()                                   # a no-op without a begin
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: term_get"):
            b.term_get()
        x, y = a.step(9, outputs=KEYS), b.step(9, outputs=KEYS)
        for k in KEYS:
            same(y[k], x[k], f"{never}, after the end: {k}")
        state_equal(b.get_state(), a.get_state(), f"{never}, after the end")


def test_after_term_end_the_context_is_plain(M, rom, oc):
    soc0, tc, rng = inputs(N)
    stop = dict(soc_stop=soc_stop(oc, rom, soc0, tc, rng))
    with M.Context(rom, N) as b, M.Context(rom, N) as twin:
        for c in (b, twin):
            setup(c, soc0, tc)
        fused(b, (20,), stop)
        b.term_end()
        twin.set_state(b.get_state())                  # a plain context started from that state
        x, y = b.step(15, outputs=KEYS), twin.step(15, outputs=KEYS)
        for k in KEYS:
            same(x[k], y[k], f"after the end: {k}")
        state_equal(b.get_state(), twin.get_state(), "after the end")


# ---- 5. step_until ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def until_ref(M, rom, oc):
    """Every cell latches within the run but one the reference kills: the open count reaches 0."""
    soc0, tc, rng = inputs(N)
    th = soc_stop(oc, rom, soc0, tc, rng, early=np.arange(N) % 7 == 0, never=np.zeros(N, dtype=bool), last=30)
    with M.Context(rom, N) as a:
        setup(a, soc0, tc)
        kill(a)
        ref = host_loop(a, NSTEPS, dict(soc_stop=th), T=tc)
    assert ref["opens"][-1] == 0 and ref["opens"][20] > 0 and ref["term"]["state"][3] == tr.DEAD
    return soc0, tc, th, ref


def kill(ctx, cell=3):
    """A NaN command through set_state: the rule finds the cell DEAD at its first step."""
    scal = ctx.get_state()["scal"]
    scal[cell, S_UK] = np.nan
    ctx.set_state({"scal": scal})


@pytest.mark.parametrize("chunk", [1, 8, 64])
def test_step_until(M, rom, until_ref, chunk):
    soc0, tc, th, ref = until_ref
    opens = ref["opens"]
    want = next((t for t in range(chunk, NSTEPS + 1, chunk) if opens[t - 1] == 0), NSTEPS)
    print(f"chunk = {chunk}: the reference's open count reaches 0 at step {opens.index(0) + 1}: steps_run = {want}")
    with M.Context(rom, N) as a, M.Context(rom, N) as b:
        for c in (a, b):
            setup(c, soc0, tc)
            kill(c)
            c.term_begin(soc_stop=th)
        run, left = b.step_until(NSTEPS, chunk=chunk)
        assert (run, left) == (want, 0)
        a.step(want, outputs=())
        state_equal(b.get_state(), a.get_state(), f"chunk = {chunk}")
        ra, rb = a.term_get(), b.term_get()
        for k in tr.FIELDS:
            same(rb[k], ra[k], f"chunk = {chunk}: term record {k}")
            if k not in ("rest",):                     # the overshoot rests on: every other field is the reference's
                same(rb[k], ref["term"][k], f"chunk = {chunk}: term record {k} vs the reference")
        assert rb["state"][3] == tr.DEAD and b.term_open() == 0


def test_step_until_cap_and_summary(M, rom, until_ref):
    soc0, tc, th, ref = until_ref
    with M.Context(rom, N) as b:
        setup(b, soc0, tc)
        kill(b)
        b.summary_begin()
        b.term_begin(soc_stop=th)
        run, left = b.step_until(21, chunk=8, tc=tc)   # 8 + 8 + 5 steps, the cap reached with cells still open
        assert (run, left) == (21, ref["opens"][20]) and left > 0
        got = b.get_summary()
        part = {k: ref[k][:21] for k in KEYS}
        sr.same_record(got, sr.reduce(part), "step_until on a summary", fields=[k for k in sr.FIELDS if not k.startswith("obs_")])
        assert b.step_until(0) == (0, left)


# ---- 6. the string flag does not depend on block scheduling -------------------------------------
def test_two_runs_of_a_pack_case_give_the_same_bits(M, rom, oc):
    soc0, tc, rng = inputs(N)
    th, _ = pack_thresholds(oc, rom, 100, soc0, tc, rng)
    outs = []
    for _ in range(2):
        with M.Context(rom, N) as b:
            setup(b, soc0, tc)
            got = fused(b, CALLS, dict(soc_stop=th), S=100)
            got["state"] = b.get_state()
        outs.append(got)
    assert (outs[0]["term"]["reason"] == 8).any()
    for k in KEYS + ("ucmd", "limiter"):
        same(outs[0][k], outs[1][k], f"run 1 vs run 2: {k}")
    for k in tr.FIELDS:
        same(outs[0]["term"][k], outs[1]["term"][k], f"run 1 vs run 2: term record {k}")
    state_equal(outs[0]["state"], outs[1]["state"], "run 1 vs run 2")


# ---- 7. refusals and the wrappers ---------------------------------------------------------------
def test_refusals_change_nothing(M, rom):
    soc0, tc, _ = inputs(24)
    with M.Context(rom, 24) as ctx:
        ctx.term_begin(soc_stop=0.9)                    # may precede init_cells
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: step_until: call mpcekf_init_cells first"):
            ctx.step_until(4)
        ctx.term_end()
        setup(ctx, soc0, tc)
        ctx.step(3, outputs=())
        st0 = ctx.get_state()
        for call in (lambda: ctx.step_until(4), ctx.term_get, ctx.term_open):
            with pytest.raises(M.MpcekfError, match="mpcekf error -5: .*call mpcekf_term_begin first"):
                call()
        L, h = ctx.L, ctx.h
        par = np.full((3, 24), np.nan)
        assert L.mpcekf_term_begin(h, par.ctypes.data_as(L.mpcekf_term_begin.argtypes[1]), 0) == -1
        assert L.mpcekf_term_begin(h, None, 1) == -1
        with pytest.raises(M.MpcekfError, match="mpcekf error -5: term_get"):   # a refused begin began nothing
            ctx.term_get()
        state_equal(ctx.get_state(), st0, "refused without a begin")
        ctx.term_begin(soc_stop=soc0 / 100.0 + 0.001)
        ctx.step(5, outputs=())
        st1, rec1 = ctx.get_state(), ctx.term_get()
        assert (rec1["state"] == 1).any()
        assert L.mpcekf_step_until(h, -1, 4, None, None, None) == -1 and b"max_steps" in L.mpcekf_last_error()
        assert L.mpcekf_step_until(h, 4, 0, None, None, None) == -1 and b"chunk" in L.mpcekf_last_error()
        ctx.thermal_begin(Cth=50.0, Rth=3.0, Tamb=25.0, ocv=M.thermal_ocv(rom))
        with pytest.raises(M.MpcekfError, match="mpcekf error -1: step_until: tc_degC on a thermal context"):
            ctx.step_until(4, tc=25.0)
        ctx.thermal_end()
        state_equal(ctx.get_state(), st1, "refused with a begin")
        for k in tr.FIELDS:
            same(ctx.term_get()[k], rec1[k], f"refused with a begin: record {k}")
        ctx.term_begin(soc_stop=0.99)                   # a second begin resets
        rec = ctx.term_get()
        assert (rec["state"] == 0).all() and (rec["steps"] == 0).all() and ctx.term_open() == 24


def test_wrappers_pass_the_rule_through(M, rom):
    n = 36
    soc0, tc, rng = inputs(n)
    th = soc0 / 100.0 + rng.uniform(0.004, 0.03, n)
    out = M.runMPC(rom, soc0, tc, 12, stop=dict(soc_stop=th))
    assert tuple(out["term"]) == tr.FIELDS and (out["term"]["state"] == 1).all()
    done = out["term"]["done_step"].astype(int)
    for c in range(n):
        assert (out["u"][done[c] - 1:, c] == 0).all() and (out["u"][:done[c] - 1, c] != 0).all()
        assert out["soc"][done[c] - 1, c] >= th[c] and (out["soc"][:done[c] - 1, c] < th[c]).all()
    s = M.run_summary(rom, soc0, tc, 40, stop=dict(soc_stop=th, chunk=4))
    assert s["steps_run"] == 4 * -(-done.max() // 4) and s["steps_run"] < 40
    for k in tr.FIELDS:
        if k != "rest":
            same(s["term"][k], out["term"][k], f"run_summary: term record {k}")
    assert (s["steps"] == s["steps_run"]).all() and (s["u_last"] == 0).all()
