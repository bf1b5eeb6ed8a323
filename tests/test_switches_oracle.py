"""CPU: the checkers of the constraint switches (initMPC.m opts.constraints,
constraintsMPC.m:15-101) pinned against each other.

The GPU tests compare the kernels with oracle/mpcekf_oracle.c bit for bit; here the C oracle's
compact constraint stack is pinned to the MATLAB-faithful numpy restatement
(oracle/oracle_np.py, cons=) over closed loops with a block switched off.
"""
import numpy as np
import pytest

import oracle_np

# SOC0 (%), TC (degC): one cell far from the target, one that reaches the voltage / eta rows.
# (A 93 % cell sits in the chaotic maxIter tail, where two restatements do not agree.)
CELLS = [(17.0, 23.0), (60.0, 25.0)]
STEPS = 150
MASKS = [(1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1)]
ALL_MASKS = [(c, v, e) for c in (0, 1) for v in (0, 1) for e in (0, 1)]


def ncon(mask):
    return (8 if mask[0] else 0) + (5 if mask[1] else 0) + (5 if mask[2] else 0) + 5


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(d)] = np.inf
    return d


@pytest.fixture(scope="module")
def c_runs(rom, oc):
    """One C-oracle closed loop per mask (both cells), shared by the cases."""
    soc0 = np.array([c[0] for c in CELLS])
    tc = np.array([c[1] for c in CELLS])
    return {m: oc.run(rom, soc0, tc, STEPS, nthreads=2, constraints=m) for m in MASKS + [(1, 1, 1)]}


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("cell", range(len(CELLS)))
def test_numpy_and_c_oracles_agree_with_a_block_off(rom, c_runs, mask, cell):
    soc0, tc = CELLS[cell]
    ref = oracle_np.run_cell(rom, soc0, tc, STEPS, cfg=dict(constraints=mask))
    out = c_runs[mask]
    for k in ("u", "v", "soc", "phise"):
        assert rel(out[k][:, cell], ref[k]).max() <= 1e-12, (mask, cell, k)
    np.testing.assert_array_equal(out["nexec"][:, cell], np.asarray(ref["nexec"], dtype=np.int32))


@pytest.mark.parametrize("mask", [(1, 1, 0), (1, 0, 0)])
def test_eta_off_changes_the_run(c_runs, mask):
    """The 60 % cell meets the eta rows within these steps: without them its command differs."""
    assert not np.array_equal(c_runs[mask]["u"], c_runs[(1, 1, 1)]["u"])


@pytest.mark.parametrize("mask", ALL_MASKS)
def test_c_oracle_iter_mpc_takes_a_compact_lambda(rom, oc, mask):
    """orc_mpc_lin with lambda [n, nC] of the mask: runs, returns finite commands and a
    lambda of the same length, for each of the eight masks."""
    n, nc = 3, ncon(mask)
    lin = np.zeros((n, 35))
    lin[:, 0:6] = [1.0, 0.9, 0.8, 0.7, 0.6, 1.0]                 # diag(A), integrator last
    lin[:, 11] = -rom.Ts / (3600 * rom.Q) * 100                   # Csoc: the integrator state
    lin[:, 13:19] = 1e-3
    lin[:, 19] = 0.02                                             # Dv
    lin[:, 20:26] = -1e-3
    lin[:, 26] = -0.01                                            # Dphi
    lin[:, 27], lin[:, 28] = 3.9, 0.12                            # bv, bphi
    uk, ne, u1, lam = oc.mpc_lin(rom, lin, np.array([50.0, 80.0, 94.0]), np.zeros(n), np.zeros((n, nc)),
                                 constraints=mask)
    assert lam.shape == (n, nc) and np.isfinite(uk).all() and (lam >= 0).all()
    assert (ne >= 0).all() and (ne <= 100).all()
    np.testing.assert_array_equal(u1, uk)
