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


# ---------------------------------------------------------------------------
# orc_mpc_lin(constraints=mask) on the edge records of tests/test_gpu_switches_edges.py
# ---------------------------------------------------------------------------
# The GPU tests compare the switched kernels with orc_mpc_lin on records edited to leave the
# fast rank-2 sweep (switch_edges.edit_records / edit_lambda).  Here, without a GPU: the C
# oracle is defined on every one of them under every mask, agrees with the MATLAB-faithful
# numpy iter_mpc where the record is finite, and does not see a disabled block's fields.
import switch_edges as se

# eight cells (SOC0 %, TC degC) x nine closed-loop steps of the numpy oracle, cell-major,
# the first 64: near-target cells (the SOC rows bind), mid-range ones (voltage / eta rows)
# and low ones (current rows); record r belongs to group r % 8 = (cell + step) % 8
EDGE_CELLS = [(94.9, 25.0), (93.0, 29.0), (85.0, 24.0), (60.0, 35.0), (17.0, 23.0), (10.0, 25.0), (88.0, 30.0),
              (30.0, 21.0)]
FINITE_GROUPS = (0, 5)       # record, warm start and hildreth.m's dense H = M (E \ M') all finite
DU_MAX_NEG = -1e7            # Ru = |F| / (2 du_max sqrt(Nc)) - sigma_min < -sigma_min: E finite, indefinite


def _mpc_dict(lin):
    return dict(a=lin[0:6], Csoc=lin[6:12], Dsoc=lin[12], Cv=lin[13:19], Dv=lin[19], Cphi=lin[20:26], Dphi=lin[26],
                bv=lin[27], bphi=lin[28])


@pytest.fixture(scope="module")
def edge_records(rom):
    """lin [64, 35], zk(end) [64], uk_1 [64], the all-on warm start [64, 23] (read-only)."""
    c = dict(oracle_np.RUNMPC_DEFAULTS)
    recs = []
    with np.errstate(all="ignore"):
        for soc0, TC in EDGE_CELLS:
            ekf = oracle_np.init_kf(rom, soc0, TC, np.diag([1.0] * rom.n + [2e6]), c["SigmaV"], c["SigmaW"])
            mpc = oracle_np.init_mpc(rom, soc0, c["Np"], c["Nc"], c["targetSOC"], c)
            cs = oracle_np.ob_step_init(rom, soc0, TC)
            uk = 0.0
            oracle_np.ob_step(uk, TC, cs)
            for _ in range(9):
                V = oracle_np.ob_step(uk, TC, cs)
                zk, _, Xind = oracle_np.iter_ekf(ekf, V, uk, TC)
                MPC, xhat = oracle_np.ekf_mats_handler(ekf, Xind, zk, TC)
                lin = np.concatenate([MPC["a"], MPC["Csoc"], [MPC["Dsoc"]], MPC["Cv"], [MPC["Dv"]], MPC["Cphi"],
                                      [MPC["Dphi"]], [MPC["bv"], MPC["bphi"]], xhat])
                recs.append((lin, zk[-1], mpc["uk_1"], np.zeros(23) if mpc["lam"] is None else np.array(mpc["lam"])))
                mpc["SOCk_1"] = zk[-1]
                uk, _ = oracle_np.iter_mpc(xhat, MPC, mpc)
    out = tuple(np.array([r[k] for r in recs[:64]], dtype=np.float64) for k in range(4))
    assert out[0].shape == (64, 35) and np.isfinite(out[0]).all()
    for a in out:
        a.setflags(write=False)
    return out


def _edited(edge_records, mask):
    lin, zend, uk1, lam = edge_records
    g = se.groups(len(lin))
    return se.edit_records(lin.copy(), g), zend, uk1, se.edit_lambda(lam[:, se.rows_of(mask)].copy(), g), g


def _bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    assert a.shape == b.shape and same.all(), (what, np.argwhere(~same)[:4].tolist())


@pytest.mark.parametrize("mask", se.ALL_MASKS)
def test_c_oracle_is_defined_on_the_edge_records(rom, oc, edge_records, mask):
    """orc_mpc_lin returns 0 (oc.mpc_lin raises otherwise) on the eight groups under every
    mask, with nexec in 0..maxIter and lambda >= 0 or NaN.  Both group-6 variants (Dsoc = NaN;
    the SOC columns times 1e160) make F, E and so DU = -E\\F NaN, and no comparison of
    iterMPC.m:62-64 holds on NaN: such a cell never enters hildreth.m (nexec = 0, uk NaN).
    The E that Cholesky rejects *inside* a QP is the finite indefinite one of a negative
    du_max (Ru < -sigma_min): every record then runs hildreth.m under every mask."""
    L, zend, uk1, l0, g = _edited(edge_records, mask)
    uk, ne, _, lam, cost = oc.mpc_lin(rom, L, zend, uk1, l0, cost=True, constraints=mask)
    assert lam.shape == (64, ncon(mask)) and ((ne >= 0) & (ne <= 100)).all()
    assert ((lam >= 0) | np.isnan(lam) | np.isinf(lam)).all()
    assert (ne[g == 6] == 0).all() and np.isnan(uk[g == 6]).all() and np.isnan(cost["J_final"][g == 6]).all()
    assert np.isfinite(uk[g == 0]).all() and np.isfinite(lam[g == 0]).all()
    lin, _, _, lam0 = edge_records
    uk, ne, _, lam = oc.mpc_lin(rom, lin, zend, uk1, lam0[:, se.rows_of(mask)], constraints=mask, du_max=DU_MAX_NEG)
    assert (ne > 0).all() and np.isfinite(uk).all() and np.isfinite(lam).all()


@pytest.mark.parametrize("mask", se.ALL_MASKS)
def test_numpy_iter_mpc_agrees_on_the_finite_groups(rom, oc, edge_records, mask):
    """Groups 0 and 5 (finite record, warm start and H): oracle_np.iter_mpc on the compact stack
    gives orc_mpc_lin's command within 1e-12 relative and its nexec.  Group 2's record is finite
    too, but its H = M (E \\ M') overflows: hildreth.m's dense H * lambda then holds inf * 0
    where orc_hildreth's defined M (X lambda) stays finite, so the dense
    restatement is no reference for it (nexec still agrees, and is checked)."""
    L, zend, uk1, l0, g = _edited(edge_records, mask)
    uk, ne, _, lam = oc.mpc_lin(rom, L, zend, uk1, l0, constraints=mask)
    c = dict(oracle_np.RUNMPC_DEFAULTS, constraints=mask)
    hit = 0
    with np.errstate(all="ignore"):
        for i in np.nonzero(np.isin(g, FINITE_GROUPS + (2,)))[0]:
            mpc = oracle_np.init_mpc(rom, 0.0, 5, 2, c["targetSOC"], c)
            mpc.update(uk_1=uk1[i], SOCk_1=zend[i], lam=l0[i].copy())
            u, info = oracle_np.iter_mpc(L[i, 29:35], _mpc_dict(L[i]), mpc)
            assert info["nexec"] == ne[i], (mask, i, g[i])
            if g[i] == 2 and mask[1]:
                continue
            assert rel([u], [uk[i]]).max() <= 1e-12, (mask, i, g[i], u, uk[i])
            hit += info["nexec"] > 0
    assert hit > 0 or mask == (0, 0, 0)


VOFF = [m for m in se.ALL_MASKS if not m[1]]
EOFF = [m for m in se.ALL_MASKS if not m[2]]


@pytest.mark.parametrize("mask,fields", [(m, "v") for m in VOFF] + [(m, "eta") for m in EOFF])
def test_c_oracle_does_not_see_a_disabled_block(rom, oc, edge_records, mask, fields):
    """constraintsMPC.m:15-101 stacks enabled blocks only and iterMPC.m forms E, F from the
    SOC rows: inf, NaN, 1e300 and -0.0 in a disabled block's record fields change no bit of
    orc_mpc_lin's uk, nexec, lambda or cost."""
    lin, zend, uk1, lam = edge_records
    l0 = lam[:, se.rows_of(mask)]
    ref = oc.mpc_lin(rom, lin, zend, uk1, l0, cost=True, constraints=mask)
    L = se.poison_block(lin.copy(), fields)
    out = oc.mpc_lin(rom, L, zend, uk1, l0, cost=True, constraints=mask)
    for k in (0, 1, 3):
        _bits(out[k], ref[k], (mask, fields, k))
    for k in ("J_uncon", "J_final", "norm_DU", "viol"):
        _bits(out[4][k], ref[4][k], (mask, fields, k))
    assert np.isfinite(ref[0]).all()
