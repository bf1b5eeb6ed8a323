"""GPU: a fused call evaluates boundzk and zk only on the steps that can be read.

Without a `zbk` (`zk`) trajectory a fused call of N steps runs k_bounds (stores zk) on its last
step only; mpcekf_get_zk's contract is "the last step's", so nothing observable may change.  The
reference is a route the rule does not alter: N calls of one step each, whose only step is their
last, so that they launch what every step launched before.  Every comparison is bitwise, NaN
positions included.

  1. fused equals stepped, nsteps in {1, 2, 7, 64, 65}, lane quad and one-lane k_cell
  2. trajectories still whole (zk + zbk, zbk only, zk only)
  3. other routes (MB, Np = 20, a switch off, per-cell limits, split k_cell, rolling flush)
  4. graph replay
  5. error cells
  6. boundzk off
  7. mpcekf_step_until
  8. launch counts
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import batch_inputs

pytestmark = pytest.mark.gpu

N = 257           # one cell past a 256-cell k_bounds block: crosses the wave and the block boundary
STEPS = (1, 2, 7, 64, 65)   # 64: the last step is a flush step; 65: right after a flush
ONE_LANE = dict(MPCEKF_QUAD_MAX=0)   # the one-lane k_cell, the bench's route
ST_ERROR = 1


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


def make(M, rom, n, seed, cfg=None, limits=None, status=None, bounds=True):
    """A context on batch_inputs(n, seed); cfg: make_config keywords."""
    ctx = M.Context(rom, n, M.make_config(bounds=bounds, **(cfg or {})))
    ctx.init_cells(*batch_inputs(n, seed))
    if limits:
        ctx.set_limits(**limits)
    if status is not None:
        st = ctx.get_state()
        st["status"] = status
        ctx.set_state(st)
    return ctx


def stepped(M, rom, n, seed, at, env=None, **kw):
    """The reference: max(at) calls of one step each; {steps: (zk, zbk, state)} for steps in at."""
    out = {}
    with _env(**(env or {})), make(M, rom, n, seed, **kw) as ctx:
        for t in range(1, max(at) + 1):
            ctx.step(1, outputs=())
            if t in at:
                out[t] = ctx.get_zk() + (ctx.get_state(),)
    return out


_REF = {}


def ref257(M, rom, route):
    """The stepped run of the N-cell case on one route, computed once and shared (read-only)."""
    if route not in _REF:
        _REF[route] = stepped(M, rom, N, 401, set(range(1, 8)) | set(STEPS) | {14},
                              env=ONE_LANE if route == "one_lane" else {})
    return _REF[route]


def check_zk(ctx, ref, what, bounds=True):
    zk, zbk = ctx.get_zk()
    same(zk, ref[0], f"{what}: zk")
    if bounds:
        same(zbk, ref[1], f"{what}: boundzk")


# ---- 1. fused equals stepped --------------------------------------------------------------------
@pytest.mark.parametrize("route", ["quad", "one_lane"])
@pytest.mark.parametrize("nsteps", STEPS)
def test_fused_equals_stepped(M, rom, route, nsteps):
    ref = ref257(M, rom, route)[nsteps]
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and (ref[1] > 0).any()
    with _env(**(ONE_LANE if route == "one_lane" else {})), make(M, rom, N, 401) as ctx:
        ctx.step(nsteps, outputs=())
        check_zk(ctx, ref, f"{route}, {nsteps} steps")
        state_equal(ctx.get_state(), ref[2], f"{route}, {nsteps} steps")


def test_routes_differ_in_launches_not_in_bits(M, rom):
    """The two references are two routes' runs of one problem: the same bits."""
    a, b = ref257(M, rom, "quad"), ref257(M, rom, "one_lane")
    for t in STEPS:
        same(a[t][0], b[t][0], f"zk at {t}")
        same(a[t][1], b[t][1], f"boundzk at {t}")


# ---- 2. trajectories still whole ----------------------------------------------------------------
@pytest.mark.parametrize("route", ["quad", "one_lane"])
@pytest.mark.parametrize("outputs", [("zk", "zbk"), ("zbk",), ("zk",)])
def test_trajectories_still_whole(M, rom, route, outputs):
    ref, nsteps = ref257(M, rom, route), 7
    with _env(**(ONE_LANE if route == "one_lane" else {})), make(M, rom, N, 401) as ctx:
        out = ctx.step(nsteps, outputs=outputs)
        for k in range(nsteps):
            if "zk" in outputs:
                same(out["zk"][k], ref[k + 1][0], f"{outputs}: zk row {k}")
            if "zbk" in outputs:
                same(out["zbk"][k], ref[k + 1][1], f"{outputs}: zbk row {k}")
        check_zk(ctx, ref[nsteps], f"{route}, {outputs}")
        zk, zbk = ctx.get_zk()
        if "zk" in outputs:
            same(zk, out["zk"][-1], "get_zk's zk vs the last row")
        if "zbk" in outputs:
            same(zbk, out["zbk"][-1], "get_zk's boundzk vs the last row")
        state_equal(ctx.get_state(), ref[nsteps][2], f"{route}, {outputs}")


# ---- 3. other routes ----------------------------------------------------------------------------
def _limits(n):
    rng = np.random.Generator(np.random.PCG64(409))
    return dict(v_max=rng.uniform(3.9, 4.1, n), phise_min=np.full(n, 0.10))


ROUTES = {
    # name: (make_config keywords, per-cell limits?, environment)
    "mb": (dict(method="MB"), False, {}),
    "np20": (dict(Np=20, Nc=10), False, {}),
    "switch_off": (dict(constraints=(1, 0, 1)), False, {}),
    "percell": ({}, True, {}),
    "percell_np20": (dict(Np=20, Nc=10), True, {}),
    "split_cell": ({}, False, dict(MPCEKF_QUAD=0, MPCEKF_SPLIT_CELL=1)),
    "flush_roll": ({}, False, dict(MPCEKF_FLUSH_ROLL=1)),
    "flush_roll_one_lane": ({}, False, dict(MPCEKF_FLUSH_ROLL=1, MPCEKF_QUAD_MAX=0)),
    # k_bounds on the side stream: no fork or join on the steps that do not launch it
    "bounds_side": ({}, False, dict(MPCEKF_BOUNDS_SIDE=65536)),
    "bounds_side_one_lane": ({}, False, dict(MPCEKF_BOUNDS_SIDE=65536, MPCEKF_QUAD_MAX=0)),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_other_routes(M, rom, route):
    cfg, percell, env = ROUTES[route]
    n, nsteps = 65, 3
    kw = dict(cfg=cfg, limits=_limits(n) if percell else None)
    ref = stepped(M, rom, n, 419, {nsteps}, env=env, **kw)[nsteps]
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    with _env(**env), make(M, rom, n, 419, **kw) as ctx:
        ctx.step(nsteps, outputs=())
        check_zk(ctx, ref, route)
        state_equal(ctx.get_state(), ref[2], route)


# ---- 4. graph replay ----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["quad", "one_lane"])
def test_graph_replay(M, rom, route):
    ref = ref257(M, rom, route)
    with _env(**(ONE_LANE if route == "one_lane" else {})), make(M, rom, N, 401) as ctx:
        ctx.set_graph(True)
        for t in (7, 14):   # the capture, then its replay
            ctx.step(7, outputs=())
            check_zk(ctx, ref[t], f"graph, {t} steps")
        state_equal(ctx.get_state(), ref[14][2], "graph, 14 steps")


# ---- 5. error cells -----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["quad", "one_lane"])
def test_error_cells(M, rom, route):
    n, nsteps, bad = 65, 6, [0, 2, 64]
    status = np.zeros(n, dtype=np.int32)
    status[bad] = ST_ERROR
    keep = np.setdiff1d(np.arange(n), bad)
    env = ONE_LANE if route == "one_lane" else {}
    clean = stepped(M, rom, n, 421, {nsteps}, env=env)[nsteps]
    with _env(**env), make(M, rom, n, 421, status=status) as ctx:
        ctx.step(nsteps, outputs=())
        zk, zbk = ctx.get_zk()
    assert np.isnan(zk[bad]).all() and np.isnan(zbk[bad]).all()
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    same(zk[keep], clean[0][keep], "zk of the other cells")
    same(zbk[keep], clean[1][keep], "boundzk of the other cells")


# ---- 6. boundzk off -----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["quad", "one_lane"])
def test_bounds_off(M, rom, route):
    nsteps = 7
    with _env(**(ONE_LANE if route == "one_lane" else {})), make(M, rom, N, 401, bounds=False) as ctx:
        ctx.set_timing(True)
        ctx.get_timing()
        ctx.step(nsteps, outputs=())
        t = ctx.get_timing()
        assert t["bounds"] == (0.0, 0), t
        assert t["hild"][1] == nsteps, t
        check_zk(ctx, ref257(M, rom, route)[nsteps], "bounds off", bounds=False)


# ---- 7. mpcekf_step_until -----------------------------------------------------------------------
def test_step_until(M, rom):
    """A rule that no cell meets: 13 steps in chunks of 5 (5 + 5 + 3), every chunk a fused call."""
    n, nsteps = 65, 13
    with make(M, rom, n, 431) as ctx:   # the rule's kernel changes no bit of an open cell
        ctx.term_begin(soc_stop=2.0)
        for _ in range(nsteps):
            ctx.step(1, outputs=())
        ref = ctx.get_zk() + (ctx.get_state(),)
    with make(M, rom, n, 431) as ctx:
        ctx.term_begin(soc_stop=2.0)
        assert ctx.step_until(nsteps, chunk=5) == (nsteps, n)
        check_zk(ctx, ref, "step_until")
        state_equal(ctx.get_state(), ref[2], "step_until")


# ---- 8. launch counts ---------------------------------------------------------------------------
def test_launch_counts(M, rom):
    nsteps = 6
    with _env(**ONE_LANE), make(M, rom, N, 401) as ctx:
        ctx.set_timing(True)
        ctx.get_timing()
        for outputs, want in (((), 1), (("zk",), 1), (("zbk",), nsteps), (("zk", "zbk"), nsteps)):
            ctx.step(nsteps, outputs=outputs)
            t = ctx.get_timing()
            assert t["bounds"][1] == want, (outputs, t)
            assert t["cell"][1] == nsteps and t["hild"][1] == nsteps, (outputs, t)
            assert t["bounds"][0] > 0.0, (outputs, t)
        ctx.step(1, outputs=())   # a control loop's call: its only step is its last
        assert ctx.get_timing()["bounds"][1] == 1
