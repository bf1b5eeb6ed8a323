"""CPU: the constraint switches at the C ABI and in the Python wrappers, on the argument
paths that end before any device call (as tests/test_abi.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

E_UNSUPPORTED = -4
ALL_MASKS = [(c, v, e) for c in (0, 1) for v in (0, 1) for e in (0, 1)]


@pytest.fixture(scope="module")
def M(P):
    return importlib.import_module("mpc-ekf4fastcharge_amd.mpcekf")


def nrows(mask, Np=5, Nc=2):
    return (4 * Nc if mask[0] else 0) + (Np if mask[1] else 0) + (Np if mask[2] else 0) + Np


def _constraints_rc(M, cfg, n=0):
    L = M._lib.load()
    rc = L.mpcekf_constraints(0, C.byref(cfg), 2.0, n, None, None, None, None, None)
    return rc, L.mpcekf_last_error().decode()


@pytest.mark.parametrize("mask", ALL_MASKS)
def test_constraints_accepts_every_mask_at_5_2(M, mask):
    rc, msg = _constraints_rc(M, M.make_config(constraints=mask))
    assert rc == 0, msg   # n = 0: the configuration check passed, nothing to compute


def test_non_zero_means_on(M):
    cfg = M.make_config(constraints=(5, -1, 0))
    assert M.constraint_rows(cfg) == nrows((1, 1, 0))
    assert _constraints_rc(M, cfg)[0] == 0


@pytest.mark.parametrize("mask", [m for m in ALL_MASKS if m != (1, 1, 1)])
def test_wide_horizon_with_a_switch_off_is_unsupported(M, rom, mask):
    cfg = M.make_config(Np=20, Nc=10, constraints=mask)
    rc, msg = _constraints_rc(M, cfg)
    assert rc == E_UNSUPPORTED
    assert "Np=20" in msg and "Nc=10" in msg and "switch" in msg
    with pytest.raises(M.MpcekfError, match=r"mpcekf error -4: Np=20 Nc=10"):
        M.Context(rom, 4, cfg)   # refused by the configuration check, before the device is touched


def test_wide_horizon_all_on_passes_the_configuration_check(M):
    assert _constraints_rc(M, M.make_config(Np=20, Nc=10))[0] == 0


def test_null_arguments_are_still_refused(M):
    rc, msg = _constraints_rc(M, M.make_config(constraints=(1, 1, 0)), n=3)
    assert rc != 0 and rc != E_UNSUPPORTED and "constraints" in msg


def test_ctx_create_no_longer_refuses_a_switch_at_5_2(M, rom):
    """With a device the context is created; without one the failure is the device's, not
    MPCEKF_E_UNSUPPORTED."""
    try:
        with M.Context(rom, 2, M.make_config(constraints=(1, 1, 0))) as ctx:
            assert ctx.ncon == 18
    except M.MpcekfError as e:
        assert "mpcekf error -4" not in str(e) and "switch" not in str(e)


@pytest.mark.parametrize("mask", ALL_MASKS)
def test_python_constraints_mpc_shapes(M, rom, mask):
    cfg = M.make_config(constraints=mask)
    Mm, g = M.constraintsMPC(np.empty((0, 35)), np.empty(0), np.empty(0), rom.Q, cfg)
    assert Mm.shape == (0, nrows(mask), 2) and g.shape == (0, nrows(mask))
    assert M.constraint_rows(cfg) == nrows(mask)
    assert 5 <= nrows(mask) <= 23
