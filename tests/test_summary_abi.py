"""CPU: the per-cell charge summary part of the C-ABI (mpcekf_summary_begin / _step_summary /
_get_summary / _summary_end) is declared, exported and bound at ABI 5; a NULL context is an
error, not a crash; the Python wrapper validates its arguments before the library is called;
the MATLAB gateway's four commands refuse bad arguments with the gateway's error identifier
before they look at the handle; and tests/summary_ref.py, the reference the GPU tests reduce
their twin's trajectories with, gives the hand-worked record on hand-made rows."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

import mexshim
import summary_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_summary_begin", "mpcekf_step_summary", "mpcekf_get_summary", "mpcekf_summary_end")
E_ARG = -1


def test_header_declares_enum_and_entry_points():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    m = re.search(r"enum \{\s*MPCEKF_SUM_SEEN = 0,(.*?)MPCEKF_NSUM\s*\}", HEADER, re.S)
    assert m, "MPCEKF_SUM_* enum"
    names = ["seen"] + [n.lower() for n in re.findall(r"MPCEKF_SUM_(\w+)", m.group(1))]
    assert tuple(names) == summary_ref.FIELDS
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)
    assert re.search(r"#define MPCEKF_SUM_WIN 64\b", HEADER)
    # the threshold's unit is stated where the field is defined
    doc = HEADER[:HEADER.index("MPCEKF_SUM_SEEN = 0")].rsplit("/*", 1)[1]
    assert "runMPC.m:109" in doc and "fraction 0..1" in doc


def test_lib_exports_and_binds(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    assert lib.ABI_VERSION == 5 == L.mpcekf_abi_version()
    for s in NEW:
        assert s in lib.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int, s
    assert lib.SUMMARY_FIELDS == summary_ref.FIELDS and lib.SUM_WIN == 64
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert M.Context.SUMMARY_FIELDS == summary_ref.FIELDS
    for name in ("summary_begin", "step_summary", "get_summary", "summary_end"):
        assert callable(getattr(M.Context, name)), name
    p = inspect.signature(M.run_summary).parameters
    assert [k for k in p][:4] == ["rom", "SOC0", "TC", "nsteps"]
    for k in ("cfg", "ncells", "tc_traj", "limits", "reach", "obs", "chunk"):
        assert p[k].default is None, k
    assert import_module("mpc-ekf4fastcharge_amd").run_summary is M.run_summary


def test_null_ctx_is_an_error(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    ids = np.array([0, 5], dtype=np.int32)
    vals = np.zeros((2, 4))
    for f, args in ((L.mpcekf_summary_begin, (None, None, -1)),
                    (L.mpcekf_step_summary, (None, 1, None)),
                    (L.mpcekf_get_summary, (None, 2, lib.iptr(ids), lib.dptr(vals))),
                    (L.mpcekf_summary_end, (None,))):
        assert f(*args) == E_ARG
        assert b"null ctx" in L.mpcekf_last_error()


def test_python_validation_needs_no_device(P):
    """On a Context object with no library context behind it: a touch of the handle would be
    an AttributeError / a crash, not the KeyError / ValueError asked for."""
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    ctx = M.Context.__new__(M.Context)
    ctx.n, ctx.h, ctx.L, ctx.rom = 5, None, None, P.make_synth_rom()
    with pytest.raises(KeyError, match="negPhise9"):
        ctx.summary_begin(obs="negPhise9")
    with pytest.raises(KeyError, match="phise"):              # a trajectory name is no obs field
        ctx.summary_begin(obs=("phise", 0))
    with pytest.raises(ValueError, match="reach must be a scalar or a length-5 array"):
        ctx.summary_begin(reach=np.full(4, 0.5))
    with pytest.raises(ValueError, match="reach must be a scalar or a length-5 array"):
        ctx.summary_begin(reach=np.full((5, 1), 0.5))
    with pytest.raises(ValueError, match="give \\(field, index\\)"):     # a vector field needs its index
        ctx.summary_begin(obs="Thetae")
    m = ctx.rom.obs_layout()["Thetae"]
    with pytest.raises(ValueError, match="give \\(field, index\\)"):
        ctx.summary_begin(obs=("Thetae", m.stop - m.start))
    with pytest.raises(ValueError, match="is a scalar"):
        ctx.summary_begin(obs=("negPhise0", 1))
    with pytest.raises(KeyError, match="u_mean"):
        ctx.get_summary(fields=("u_min", "u_mean"))
    # what does pass
    lay = ctx.rom.obs_layout()
    r, slot = ctx._summary_args(0.5, "negPhise0")
    assert r.dtype == np.float64 and r.shape == (5,) and r.flags.c_contiguous and (r == 0.5).all()
    assert slot == lay["negPhise0"].start
    assert ctx._summary_args(None, ("Thetae", 1)) == (None, lay["Thetae"].start + 1)
    assert ctx._summary_args(None, None) == (None, -1)
    ctx.h = None


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)


def test_gateway_summary_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, a slot that is no 1-based integer,
    a reach that is no double array, an nsteps that is no count: all mpcekf:arg, and none
    dereferences the handle."""
    ok = {"summarybegin": (np.zeros((0, 0)), 0.0), "stepsummary": (2.0,), "getsummary": (), "summaryend": ()}
    for cmd, args in ok.items():
        out = 1 if cmd == "getsummary" else 0
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=out)
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=out)
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=out)
    for cmd in ("summarybegin", "stepsummary", "summaryend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: getsummary: at most 1 output"):
        shim.mex("getsummary", DEAD, nargout=2)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: summarybegin: slot = .* is not a slot 1..nobs"):
            shim.mex("summarybegin", DEAD, np.zeros((0, 0)), bad, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: summarybegin: slot: expected a real numeric scalar"):
        shim.mex("summarybegin", DEAD, np.zeros((0, 0)), np.array([[1.0, 2.0]]), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: summarybegin: reach: expected"):
        shim.mex("summarybegin", DEAD, np.zeros((1, 4), dtype=np.int32), 0.0, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepsummary', h, nsteps"):
        shim.mex("stepsummary", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepsummary", DEAD, bad, nargout=0)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd


# ---- summary_ref on hand-made rows ----------------------------------------------------------
NaN = float("nan")


def _rows():
    """6 steps x 4 cells.
    cell 0: a NaN step (step 3: v is NaN) between counted ones; reaches 0.5 at step 4.
    cell 1: ties -- u's minimum and v's maximum occur twice: the first occurrence wins.
    cell 2: a +0 / -0 pair in u and phise: neither displaces the other; threshold never reached.
    cell 3: NaN from the first step on (a cell in error)."""
    u = np.array([[-3.0, -5.0, 0.0, NaN],
                  [-4.0, -7.0, -0.0, NaN],
                  [-9.0, -7.0, 0.0, NaN],
                  [-2.0, -6.0, -0.0, NaN],
                  [-4.0, -1.0, 0.0, NaN],
                  [-1.0, -2.0, -0.0, NaN]])
    v = np.array([[3.5, 3.6, 3.0, NaN],
                  [3.7, 3.9, 3.0, NaN],
                  [NaN, 3.8, 3.0, NaN],
                  [3.6, 3.9, 3.0, NaN],
                  [3.9, 3.7, 3.0, NaN],
                  [3.8, 3.5, 3.0, NaN]])
    soc = np.array([[0.1, 0.1, 0.1, NaN],
                    [0.2, 0.2, 0.1, NaN],
                    [0.6, 0.3, 0.1, NaN],
                    [0.5, 0.4, 0.1, NaN],
                    [0.7, 0.5, 0.1, NaN],
                    [0.8, 0.6, 0.1, NaN]])
    ph = np.array([[0.3, 0.2, -0.0, NaN],
                   [0.2, 0.1, 0.0, NaN],
                   [0.0, 0.1, -0.0, NaN],
                   [0.25, 0.3, 0.0, NaN],
                   [0.1, 0.3, -0.0, NaN],
                   [0.4, 0.3, 0.0, NaN]])
    ne = np.array([[0, 1, 0, 0],
                   [5, 100, 0, 0],
                   [100, 7, 0, 0],
                   [100, 100, 0, 0],
                   [2, 0, 0, 0],
                   [0, 120, 0, 0]], dtype=np.int32)
    obs = np.array([[0.5, NaN, 0.0, NaN],
                    [0.4, 0.2, -0.0, NaN],
                    [0.1, 0.2, 0.0, NaN],     # cell 0: the plant's slot is not NaN at the uncounted step
                    [NaN, 0.1, -0.0, NaN],
                    [0.9, 0.1, 0.0, NaN],
                    [0.9, 0.3, -0.0, NaN]])
    return dict(u=u, v=v, soc=soc, phise=ph, nexec=ne), obs


def _col(r, c):
    return {k: r[k][c] for k in summary_ref.FIELDS}


def _same(got, want):
    for k, w in want.items():
        g = got[k]
        assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64), (k, g, w)


def test_summary_ref_on_hand_made_rows():
    traj, obs = _rows()
    reach = np.array([0.5, 0.45, 0.9, 0.0])
    r = summary_ref.reduce(traj, reach=reach, obs=obs, max_hild=100)
    assert tuple(r) == summary_ref.FIELDS and all(v.shape == (4,) and v.dtype == np.float64 for v in r.values())
    # cell 0: step 3 is not counted (its soc 0.6 >= 0.5 does not reach; its nexec 100 is not summed)
    _same(_col(r, 0), dict(seen=6.0, steps=5.0, err_step=3.0, t_reach=4.0, u_min=-4.0, u_min_step=2.0, u_max=-1.0,
                           v_max=3.9, v_max_step=5.0, v_min=3.5, phise_min=0.1, phise_min_step=5.0, u_last=-1.0,
                           v_last=3.8, soc_last=0.8, phise_last=0.4, u_sum=((((-3.0 + -4.0) + -2.0) + -4.0) + -1.0),
                           nexec_sum=107.0, nexec_max=100.0, nsat=1.0, obs_min=0.1, obs_min_step=3.0, obs_max=0.9,
                           obs_max_step=5.0))
    # cell 1: ties keep the first occurrence; nexec 120 >= max_hild counts as saturated
    _same(_col(r, 1), dict(seen=6.0, steps=6.0, err_step=0.0, t_reach=5.0, u_min=-7.0, u_min_step=2.0, u_max=-1.0,
                           v_max=3.9, v_max_step=2.0, v_min=3.5, phise_min=0.1, phise_min_step=2.0, u_last=-2.0,
                           phise_last=0.3, nexec_sum=328.0, nexec_max=120.0, nsat=3.0, obs_min=0.1, obs_min_step=4.0,
                           obs_max=0.3, obs_max_step=6.0))
    # cell 2: +0 first in u (stays +0), -0 first in phise and +0 first in obs (stay); never reaches 0.9
    _same(_col(r, 2), dict(steps=6.0, t_reach=0.0, u_min=0.0, u_min_step=1.0, u_max=0.0, phise_min=-0.0,
                           phise_min_step=1.0, u_last=-0.0, phise_last=0.0, u_sum=0.0, obs_min=0.0, obs_min_step=1.0,
                           obs_max=0.0, obs_max_step=1.0, nexec_max=0.0, nsat=0.0))
    # cell 3: no counted step -- extrema and last values NaN, step fields and sums 0; a threshold of 0 is not reached
    _same(_col(r, 3), dict(seen=6.0, steps=0.0, err_step=1.0, t_reach=0.0, u_min=NaN, u_min_step=0.0, u_max=NaN,
                           v_max=NaN, v_max_step=0.0, v_min=NaN, phise_min=NaN, phise_min_step=0.0, u_last=NaN,
                           v_last=NaN, soc_last=NaN, phise_last=NaN, u_sum=0.0, nexec_sum=0.0, nexec_max=NaN,
                           nsat=0.0, obs_min=NaN, obs_min_step=0.0, obs_max=NaN, obs_max_step=0.0))
    # no threshold, no slot
    r0 = summary_ref.reduce(traj)
    assert (r0["t_reach"] == 0).all() and np.isnan(r0["obs_min"]).all() and (r0["obs_max_step"] == 0).all()
    # accumulation: 2 + 1 + 3 steps continue the step index and give the one-pass record
    part = None
    for a, b in ((0, 2), (2, 3), (3, 6)):
        part = summary_ref.reduce({k: x[a:b] for k, x in traj.items()}, reach=reach, obs=obs[a:b], state=part)
    summary_ref.same_record(part, r, "2 + 1 + 3 steps")
    with pytest.raises(AssertionError, match="u_last"):
        summary_ref.same_record(dict(r, u_last=np.abs(r["u_last"])), r, "sign of zero")
