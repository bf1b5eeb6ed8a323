"""CPU: the EKF measurement update's Jacobi symmetrisation and Q-bump (iterEKF.m:141-151 /
164-173) on the two oracles.

The C oracle counts its branch hits (oracle_c.branch_counts); the cases of tests/ekf_branches.py
are asserted to be on the branches, the default configuration to be off them, and on the
branches the C oracle (LDL' shortcut, cyclic Jacobi) is held to the MATLAB-faithful numpy
restatement (LAPACK svd, no shortcut) within the project's C-vs-numpy bound 1e-12.
"""
import numpy as np
import pytest

import ekf_branches as B

RTOL_C_NUMPY = 1e-12


@pytest.mark.parametrize("name", [k for k in B.CASES if k != "default"])
def test_case_reaches_its_branches(name):
    """Every configuration the GPU tests run is on the branch it is there for (floors at about
    half the measured shares, tests/ekf_branches.py)."""
    ref, bc = B.oracle(name)
    B.check_floors(name, bc)
    if name != "x0-huge":   # the comparison is on finite data (x0-huge: its error cells are NaN)
        assert (ref["status"] == 0).all()
        for k in ("u", "v", "soc", "phise", "x", "zk_traj", "zbk_traj"):
            assert np.isfinite(ref[k]).all(), k
    else:
        bad = ref["status"] != 0
        assert 0 < bad.sum() < bad.size and np.isfinite(ref["u"][:, ~bad]).all()


def test_default_configuration_never_reaches_the_branches():
    """runMPC.m's SigmaV / SigmaX0, 64 cells x 100 steps: not one non-PD update, not one bump.
    Why the cases above exist: no workload of the suite at the default tuning compares anything
    on these branches."""
    _, bc = B.oracle("default")
    assert bc["updates"] == 64 * 100 * 4 and bc["nonpd"] == 0 and bc["bump"] == 0 and bc["both"] == 0, bc


def test_branch_counts_reset_and_do_not_change_results(rom, oc):
    soc0, tc = B.cells("sigv-linear")
    a, bc = B.counts_of(oc, lambda: oc.run(rom, soc0[:4], tc[:4], 30, nthreads=2, SigmaV=1e-5))
    assert bc["ob"]["updates"] == 4 * 30 * 4 and bc["mb"]["updates"] == 0
    assert oc.branch_counts() == {f: dict(updates=0, nonpd=0, bump=0, both=0) for f in ("ob", "mb")}
    b = oc.run(rom, soc0[:4], tc[:4], 30, nthreads=1, SigmaV=1e-5)
    for k in ("u", "v", "soc", "phise", "nexec"):
        np.testing.assert_array_equal(a[k], b[k])


# measured on the first 4 cells x 100 steps: sigv OB non-PD 8.4 % (134 of 1,600), bump 8.8 %;
# sigv MB bump 3.75 % (15 of 400, no non-PD); x0zero OB non-PD 3.0 % (48 of 1,600, all in steps
# 1-5); x0zero MB non-PD 3.5 % (14 of 400)
@pytest.mark.parametrize("method,cfg,floors", [
    ("OB", dict(SigmaV=1e-5), dict(nonpd=0.04, bump=0.04)),
    ("MB", dict(SigmaV=1e-5), dict(bump=0.018)),
    ("OB", dict(SigmaX0=B.X0_ZERO), dict(nonpd=0.015)),
    ("MB", dict(SigmaX0=B.X0_ZERO), dict(nonpd=0.017)),
])
def test_c_oracle_matches_numpy_on_the_branches(rom, oc, method, cfg, floors):
    """oc.run against oracle_np.run_cell, first 4 batch cells x 100 steps."""
    import oracle_np as O
    soc0, tc = B.cells("sigv-linear")
    soc0, tc = soc0[:4], tc[:4]
    r, bc = B.counts_of(oc, lambda: oc.run(rom, soc0, tc, 100, nthreads=4, method=method, **cfg))
    B.check_floors(f"{method} {cfg}", bc[method.lower()], floors)
    worst = 0.0
    for i in range(4):
        o = O.run_cell(rom, soc0[i], tc[i], 100, dict(cfg, method=method))
        for k in ("u", "v", "soc", "phise"):
            assert np.isfinite(o[k]).all(), k
            worst = max(worst, B.rel(r[k][:, i], o[k]).max())
        np.testing.assert_array_equal(r["nexec"][:, i], o["nexec"])
    print(f"{method} {cfg}: max rel C vs numpy {worst:.3e}")
    assert worst <= RTOL_C_NUMPY


@pytest.mark.parametrize("fixture,floors", B.GOLDEN)
def test_c_oracle_matches_branch_fixtures(rom, oc, fixture, floors):
    """The numpy restatement's branch fixtures (tools/make_golden.py --branches-only) hold the
    C oracle to 1e-12."""
    g = B.golden(fixture)
    assert B.rom_hash(rom) == str(g["rom_hash"])
    cfg = B.golden_cfg(g)
    r, bc = B.counts_of(oc, lambda: oc.run(rom, g["soc0"], g["tc"], g["u"].shape[0], nthreads=4, **cfg))
    B.check_floors(fixture, bc[cfg["method"].lower()], floors)
    np.testing.assert_array_equal(r["status"], g["status"])
    for k in ("u", "v", "soc", "phise"):
        assert np.isfinite(g[k]).all()
        assert B.rel(r[k], g[k]).max() <= RTOL_C_NUMPY, (k, B.rel(r[k], g[k]).max())
    np.testing.assert_array_equal(r["nexec"], g["nexec"])


def test_numpy_default_sigmax0_is_unchanged(rom):
    """cfg["SigmaX0"] left out is runMPC.m's (1,1,1,1,1,2e6): the same bits as naming it."""
    import oracle_np as O
    a = O.run_cell(rom, 17.0, 23.0, 40)
    b = O.run_cell(rom, 17.0, 23.0, 40, {"SigmaX0": (1, 1, 1, 1, 1, 2e6)})
    for k in ("u", "v", "soc", "phise", "zbk"):
        np.testing.assert_array_equal(a[k], b[k])
