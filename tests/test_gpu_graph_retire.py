"""GPU: a graph cached before an extension's _end is not replayed after the matching _begin
(mpcekf_set_graph; the graph cache of the fused step and the retirement every _end does).

Two contexts of one configuration run one sequence, A with graphs off and B with graphs on.  For
each of pack, coupling, balancer, charger, termination, aging, thermal schedule and summary in
turn: begin every extension, three calls of 4 steps (B captures a graph and replays it twice), end
that one extension and begin it again with other parameter values, three calls of 4 steps again.
Every row the calls return, every record and the state of A and B are equal bit for bit; on A the
two halves of every turn differ, so the equality is not that of two constant runs.  The shape is
the smallest that has strings and neighbours: 8 cells in strings of 4, Np = 5 / Nc = 2, the
thermal model on.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CALLS, STEPS = 8, 3, 4
KEYS = ("u", "v", "soc", "phise", "nexec")
SOC0 = np.array([12.0, 18.0, 25.0, 30.0, 15.0, 22.0, 28.0, 35.0])   # %: more than dz_on apart inside a string
PLATING = dict(i0=1e-3, U=0.0, alpha=0.5, Ea=0.0, gate=0.12)
SEI = dict(i0=1e-6, U=0.4, alpha=0.3, Ea=5.0e4)
LATCH = np.where(np.arange(N) == 5, 0.0, 2.0)                          # cell 5 latches at once, and its string with it

# per extension: (begin, end, the first half's arguments, the second half's)
EXT = {
    "pack": (lambda c, p: c.pack_begin(p), "pack_end", 4, 2),
    "couple": (lambda c, p: c.thermal_couple(p), "thermal_couple_end", 2.0, np.linspace(0.3, 1.0, N)),
    "balance": (lambda c, p: c.balance_begin(p, 0.01, 0.005), "balance_end", 3.0, np.linspace(4.0, 9.0, N)),
    "charger": (lambda c, p: c.charger_begin(*p), "charger_end", (25.0, 400.0), (12.0, 150.0)),
    "term": (lambda c, p: c.term_begin(soc_stop=p), "term_end", 2.0, LATCH),
    "aging": (lambda c, p: c.aging_begin(p, sources=("est", "plant")), "aging_end", (PLATING, SEI), (SEI,)),
    "sched": (lambda c, p: c.thermal_schedule(20.0, 40.0, Crate=p), "thermal_schedule_end", [2.0, 1.2], [1.2, 0.6]),
    "summary": (lambda c, p: c.summary_begin(reach=p, obs="negPhise0"), "summary_end", 0.5, 0.2),
}
ENDS_TOO = {"pack": ("couple", "balance", "charger")}                  # what pack_end ends with the pack


@pytest.fixture(scope="module")
def rom(P):
    return P.make_synth_rom(lookup="quintic")


def begin(ctx, name, second=False):
    fn, _, first, other = EXT[name]
    fn(ctx, other if second else first)


def calls(ctx, name):
    """Three calls of 4 steps through the entry point that returns the turn's extension's rows."""
    if name == "summary":
        for _ in range(CALLS):
            ctx.step_summary(STEPS)
        return {}
    if name in ("couple", "aging"):
        kw = dict(thermal=("temp", "heat", "cond"), pack=("ucmd", "limiter"), aging=("rate",))
    else:
        kw = dict(thermal=("temp", "heat"), pack=("ucmd", "limiter", "bleed", "zmin", "vstr", "istr", "capby"))
    parts = [ctx.step(STEPS, outputs=KEYS, **kw) for _ in range(CALLS)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def records(ctx):
    return dict(pack=ctx.pack_get(), couple=ctx.thermal_couple_get(), balance=ctx.balance_get(),
                charger=ctx.charger_get(), term=ctx.term_get(), aging=ctx.aging_record(), thermal=ctx.thermal_get(),
                summary=ctx.get_summary(), limits=ctx.get_limits(), state=ctx.get_state())


def sequence(M, rom, graph):
    """{(extension, half): (rows, records)} of the whole sequence on one context."""
    got = {}
    with M.Context(rom, N) as ctx:
        ctx.init_cells(SOC0, 25.0)
        ctx.thermal_begin(Cth=30.0, Rth=3.0, Tamb=25.0, ocv=M.thermal_ocv(rom))
        ctx.set_graph(graph)
        for name in EXT:
            for k in EXT:
                begin(ctx, k)
            got[name, 0] = calls(ctx, name), records(ctx)
            getattr(ctx, EXT[name][1])()
            for k in (name,) + ENDS_TOO.get(name, ()):
                begin(ctx, k, second=k == name)
            got[name, 1] = calls(ctx, name), records(ctx)
    return got


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def equal(x, y):
    """Bit for bit over a tree of dicts, lists and arrays (a NaN equals only the same NaN)."""
    if isinstance(x, dict):
        return set(x) == set(y) and all(equal(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(equal(p, q) for p, q in zip(x, y))
    return np.array_equal(bits(x), bits(y))


def differing(x, y, what):
    if isinstance(x, dict):
        assert set(x) == set(y), what
        return [d for k in x for d in differing(x[k], y[k], f"{what}: {k}")]
    if isinstance(x, (list, tuple)):
        assert len(x) == len(y), what
        return [d for i, (p, q) in enumerate(zip(x, y)) for d in differing(p, q, f"{what}: {i}")]
    return [] if np.array_equal(bits(x), bits(y)) else [what]


def test_no_graph_survives_an_end(M, rom):
    a, b = sequence(M, rom, graph=False), sequence(M, rom, graph=True)
    assert list(a) == list(b) and len(a) == 2 * len(EXT)
    for name in EXT:
        # not vacuous: the halves differ on the graph-free context
        (rows0, rec0), (rows1, rec1) = a[name, 0], a[name, 1]
        if name == "summary":
            assert not equal(rec0["summary"], rec1["summary"]), name
        else:
            assert any(rows0[k].shape != rows1[k].shape or not equal(rows0[k], rows1[k]) for k in rows0), name
    for key in a:
        bad = differing(a[key][0], b[key][0], "rows") + differing(a[key][1], b[key][1], "records")
        assert not bad, f"{key[0]}, half {key[1]}: graph on differs from graph off in {bad}"
