"""GPU: the EKF measurement update's Jacobi symmetrisation and Q-bump (iterEKF.m:141-151 /
164-173) on finite data.

runMPC.m's filter tuning never leaves the positive-definite shortcut, so no other test of the
suite runs jacobi5 / jacobi6, meas_polar / meas_polar_slow, the mixed-wave reconstruction or
the bump's doubling on anything but lock-out cells.  The configurations of tests/ekf_branches.py
reach them through the ordinary initKF arguments (SigmaV, SigmaX0).  Every case first asserts,
on the C oracle's branch counters, that it is on the branch, then compares every per-step store
(u, v, soc, phise, nexec, x, zk and zbk = r' Sigma r, the one output that sees every entry of
Sigma) and the final status with the C oracle BITWISE, NaN patterns included.
"""
import numpy as np
import pytest

import ekf_branches as B

pytestmark = pytest.mark.gpu

RTOL_TIGHT = 1e-9
PAIRS = dict(u="u", v="v", soc="soc", phise="phise", nexec="nexec", x="x", zk="zk_traj", zbk="zbk_traj")
PATH_ENV = ("MPCEKF_QUAD", "MPCEKF_QUAD_MAX", "MPCEKF_SPLIT_CELL", "MPCEKF_EKF4_BLOCK")


def _bitwise(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {a[i]!r} vs {b[i]!r} "
                             f"(max rel {B.rel(a, b).max():.3e})")


def _set_path(monkeypatch, env):
    """The kernel mapping overrides are read at context creation; anything not named is the default."""
    for k in PATH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _context(M, name):
    lookup, _, _, cfg, _ = B.CASES[name]
    soc0, tc = B.cells(name)
    ctx = M.Context(B.rom(lookup), len(soc0), M.make_config(bounds=True, **cfg))
    ctx.init_cells(soc0, tc)
    return ctx


def _compare(out, ref, what, first=0):
    for k, rk in PAIRS.items():
        _bitwise(out[k], ref[rk][first:], f"{what} {k}")


# case, kernel mapping, what the mapping runs
FUSED = [
    ("sigv-linear", {}, "k_ekf4: out-of-line Jacobi under the wave vote, sparse non-PD lanes, bump"),
    ("sigv-quintic", {}, "the same on the v3 tables"),
    ("sigv-linear", dict(MPCEKF_QUAD=0), "k_cell: inline Jacobi, a lane per cell"),
    ("x0zero", dict(MPCEKF_QUAD=1), "k_ekf4, waves that mix many non-PD lanes with PD ones"),
    ("x0zero", dict(MPCEKF_QUAD=0), "k_cell, the same"),
    ("x0zero-3", dict(MPCEKF_QUAD=1), "k_ekf4, one partial wave"),
    ("x0zero-3", dict(MPCEKF_QUAD=0), "k_cell, one partial wave"),
    ("x0zero-65", dict(MPCEKF_QUAD=1), "k_ekf4, a second block of one quad"),
    ("x0zero-65", dict(MPCEKF_QUAD=0), "k_cell, a second wave of one lane"),
    ("sigv-9000", {}, "the k_cell grid above the quad limit: many waves, most of them all-PD"),
    ("mb-x0zero", {}, "MB filter: is_pd6 / jacobi6"),
    ("mb-sigv", {}, "MB filter: the bump"),
    ("wide-x0zero", {}, "Np = 20 / Nc = 10"),
    ("switched-sigv", {}, "k_cell<P_EKF | P_LIN> and the switch kernels"),
    ("sigv-40", dict(MPCEKF_SPLIT_CELL=1, MPCEKF_QUAD=0), "k_cell as two kernels"),
    ("x0-tiny", {}, "SigmaX0 = 1e-12: rare non-PD updates at a tiny scale"),
    ("x0-huge", {}, "SigmaX0 = 1e10: dense non-PD updates, bumps, cells that end in error"),
]


@pytest.mark.parametrize("name,env", [(n, e) for n, e, _ in FUSED],
                         ids=[n + "".join(f"-{k[7:].lower()}{v}" for k, v in e.items()) for n, e, _ in FUSED])
def test_fused_loop_on_the_branches_matches_oracle(M, monkeypatch, name, env):
    ref, bc = B.oracle(name)
    B.check_floors(name, bc)
    _set_path(monkeypatch, env)
    steps = B.CASES[name][2]
    with _context(M, name) as ctx:
        out = ctx.step(steps, outputs=tuple(PAIRS))
        status = ctx.get_state()["status"]
    _bitwise(status, ref["status"], f"{name} status")
    _compare(out, ref, name)
    if name == "x0-huge":   # its error cells' status words and NaN patterns were part of the comparison
        assert (status != 0).any() and np.isnan(out["zbk"][-1][status != 0]).all()
    else:
        assert (status == 0).all() and np.isfinite(out["zbk"]).all()


@pytest.mark.parametrize("asynchronous", [False, True])
def test_stage_route_on_the_branches_equals_fused(M, monkeypatch, asynchronous):
    """OB_step -> iterEKF -> EKFmatsHandler -> iterMPC through the stage ABI (host round trips,
    or the _async twins with the device hand-offs) at SigmaV = 1e-5, 64 cells x 40 steps: v, u,
    zk, boundzk and nexec of every step are the fused step's bits, which are the oracle's."""
    name = "sigv-40"
    ref, bc = B.oracle(name)
    B.check_floors(name, bc)
    _set_path(monkeypatch, {})
    steps = B.CASES[name][2]
    with _context(M, name) as ctx:
        fused = ctx.step(steps, outputs=tuple(PAIRS))
    _compare(fused, ref, name)
    with _context(M, name) as ctx:
        uk = np.zeros(ctx.n)
        for k in range(steps):
            if asynchronous:
                ctx.asynchronous = True
                v = ctx.OB_step(uk)
                zk, zb, _ = ctx.iterEKF(None, uk, xind=False)
                ctx.EKFmatsHandler(None, None, keep=True)
                ctx.asynchronous = False
                uk, ne = ctx.iterMPC(None, None)   # synchronous: completes the step's outputs
            else:
                v = ctx.OB_step(uk)
                zk, zb, xind = ctx.iterEKF(v, uk)
                lin = ctx.EKFmatsHandler(zk, xind)
                uk, ne = ctx.iterMPC(lin, zk[:, -1])
            for got, key in ((v, "v"), (uk, "u"), (zk, "zk"), (zb, "zbk"), (ne, "nexec")):
                _bitwise(got, fused[key][k], f"step {k} {key}")


def test_checkpoint_on_the_branch_is_exact(M, monkeypatch):
    """get_state at step 10 of the zero-SigmaX0 run (its records then hold reconstructed
    V|Lambda|V', not a propagated diagonal), set_state into a fresh context, on to step 40: the
    uninterrupted run's bits, and the oracle's."""
    name = "x0zero-40"
    ref, bc = B.oracle(name)
    B.check_floors(name, bc)
    _set_path(monkeypatch, {})
    with _context(M, name) as ctx:
        head = ctx.step(10, outputs=tuple(PAIRS))
        snap = ctx.get_state()
        a = ctx.step(30, outputs=tuple(PAIRS))
        end_a = ctx.get_state()
    with _context(M, name) as ctx:
        ctx.set_state(snap)
        b = ctx.step(30, outputs=tuple(PAIRS))
        end_b = ctx.get_state()
    for k in PAIRS:
        _bitwise(b[k], a[k], f"restored {k}")
        _bitwise(head[k], ref[PAIRS[k]][:10], f"head {k}")
    _compare(b, ref, "restored", first=10)
    for k in end_a:
        _bitwise(end_b[k], end_a[k], f"final state {k}")


@pytest.mark.parametrize("fixture,floors", B.GOLDEN)
def test_gpu_matches_branch_fixtures(M, oc, monkeypatch, fixture, floors):
    """Against the MATLAB-faithful numpy restatement (LAPACK svd, no PD shortcut) on the
    branches: 1e-9 on u, v, soc, phise (the project's bar for well-conditioned fixtures; the
    C oracle sits within 1e-14 of them), nexec exact."""
    g = B.golden(fixture)
    rom = B.rom("linear")
    assert B.rom_hash(rom) == str(g["rom_hash"])
    cfg = B.golden_cfg(g)
    steps = g["u"].shape[0]
    _, bc = B.counts_of(oc, lambda: oc.run(rom, g["soc0"], g["tc"], steps, nthreads=4, **cfg))
    B.check_floors(fixture, bc[cfg["method"].lower()], floors)
    _set_path(monkeypatch, {})
    out = M.runMPC(rom, g["soc0"], g["tc"], steps, cfg=M.make_config(**cfg))
    np.testing.assert_array_equal(out["status"], g["status"])
    for k in ("u", "v", "soc", "phise"):
        err = B.rel(out[k], g[k]).max()
        print(f"{fixture} {k}: max rel {err:.3e}")
        assert err <= RTOL_TIGHT, (k, err)
    np.testing.assert_array_equal(out["nexec"], g["nexec"])
