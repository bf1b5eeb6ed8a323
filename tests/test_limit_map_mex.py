"""CPU: the MATLAB gateway's 'limitmap' / 'limitmapget' / 'limitmapend' / 'stepexmap' refuse bad
arguments before they look at the handle (through the MEX API shim, tests/mex), and the session
wrapper has their ops."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
EMPTY = np.zeros((0, 0))


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_map_commands_check_arguments(shim):
    idx = np.array([2.0, 7.0])
    tab = np.asfortranarray(np.ones((5, 3, 2, 2)))            # nz x nt x 2 fields x 2 maps
    full = (idx, 0.2, 0.8, 25.0, 40.0, tab)
    ok = {"limitmap": full, "limitmapget": (), "limitmapend": (), "stepexmap": (3.0,)}
    for cmd, args in ok.items():
        nout = 1 if cmd == "limitmapget" else 6 if cmd == "stepexmap" else 0
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout)
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout)
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=0)
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: (no output|at most {nout} output)"):
            shim.mex(cmd, DEAD, *args, nargout=nout + 1)
    S = "mpcekf:arg: limitmap: "
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'limitmap', h, idx, z_lo, z_hi, T_lo, T_hi, tables"):
        shim.mex("limitmap", DEAD, *full[:-1], nargout=0)
    for bad in (EMPTY, np.arange(2.0, 9.0)):
        with pytest.raises(shim.MexError, match=S + r"idx: expected 1\.\.6 field numbers"):
            shim.mex("limitmap", DEAD, bad, *full[1:], nargout=0)
    for bad, j in ((np.array([1.0, 2.0]), 1), (np.array([2.0, 8.0]), 2), (np.array([2.5]), 1), (np.array([2.0, np.nan]), 2)):
        with pytest.raises(shim.MexError, match=S + rf"idx\({j}\) = .* is not a field that can be mapped \(2\.\.7\)"):
            shim.mex("limitmap", DEAD, bad, *full[1:], nargout=0)
    with pytest.raises(shim.MexError, match=S + r"idx\(2\) = 7 is given twice"):
        shim.mex("limitmap", DEAD, np.array([7.0, 7.0]), *full[1:], nargout=0)
    with pytest.raises(shim.MexError, match=S + "z_lo: expected a real numeric scalar"):
        shim.mex("limitmap", DEAD, idx, np.array([0.2, 0.3]), 0.8, 25.0, 40.0, tab, nargout=0)
    with pytest.raises(shim.MexError, match=S + "z_hi: expected a real numeric scalar"):
        shim.mex("limitmap", DEAD, idx, 0.2, EMPTY, 25.0, 40.0, tab, nargout=0)
    with pytest.raises(shim.MexError, match=S + "T_lo: expected a real numeric scalar"):      # a temperature axis needs its ends
        shim.mex("limitmap", DEAD, idx, 0.2, 0.8, EMPTY, 40.0, tab, nargout=0)
    for bad in (tab.astype(np.float32), EMPTY):
        with pytest.raises(shim.MexError, match=S + "tables: expected a real double nz x nt x 2 x nsets array"):
            shim.mex("limitmap", DEAD, idx, 0.2, 0.8, 25.0, 40.0, bad, nargout=0)
    for bad in (np.asfortranarray(np.ones((1, 1, 2))), np.asfortranarray(np.ones((5, 3, 3)))):   # one node; 3 tables for 2 fields
        with pytest.raises(shim.MexError, match=S + r"tables: \d x \d x \d: expected 2 or more nodes on one axis and 2 tables per map"):
            shim.mex("limitmap", DEAD, idx, 0.2, 0.8, 25.0, 40.0, bad, nargout=0)
    for bad in (2.0, 0.5, np.nan):
        with pytest.raises(shim.MexError, match=S + r"interp = .*: 0 \(linear\) or 1 \(hold\)"):
            shim.mex("limitmap", DEAD, *full, bad, nargout=0)
    with pytest.raises(shim.MexError, match=S + r"sets: expected \[\] or ncells real doubles"):
        shim.mex("limitmap", DEAD, *full, 1.0, np.ones((1, 4), dtype=np.int32), nargout=0)
    for bad, j in ((np.array([1.0, 0.0]), 2), (np.array([3.0]), 1), (np.array([1.0, 2.0, 1.5]), 3), (np.array([np.nan]), 1)):
        with pytest.raises(shim.MexError, match=S + rf"sets\({j}\) = .* is not a map 1\.\.2"):
            shim.mex("limitmap", DEAD, *full, 1.0, bad, nargout=0)
    with pytest.raises(shim.MexError, match=S + r"z0: expected \[\] or ncells real doubles"):
        shim.mex("limitmap", DEAD, *full, 0.0, EMPTY, np.ones((1, 4), dtype=np.int32), nargout=0)
    # what passes every check reaches the handle: [] for the optional arguments, no temperature axis
    for args in (full + (EMPTY, EMPTY, EMPTY), full + (1.0, np.array([1.0, 2.0, 2.0]), np.array([0.1, np.nan, 0.3])),
                 (idx, 0.2, 0.8, EMPTY, EMPTY, np.asfortranarray(np.ones((5, 1, 2))), 1.0)):
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex("limitmap", DEAD, *args, nargout=0)
    for bad in (-1.0, 2.5, np.nan):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexmap", DEAD, bad, nargout=6)
    with pytest.raises(shim.MexError, match=r"mpcekf:arg: stepexmap: tc: expected \[\] or ncells x nsteps real doubles"):
        shim.mex("stepexmap", DEAD, 3.0, np.ones((2, 3), dtype=np.float32), nargout=6)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
        assert f"mpcekf_mex('{cmd}'" in src[:src.index("#include")], f"{cmd} is in the gateway's usage comment"


def test_session_has_the_map_ops():
    src = open(os.path.join(ROOT, "matlab", "dropin", "mpcekf_session.m")).read()
    for op in ("limitmap", "limitmapget", "limitmapend", "stepexmap"):
        assert f"case '{op}'" in src and f"mpcekf_mex('{op}', P.h" in src and f"mpcekf_session('{op}'" in src, op
