"""CPU: the MATLAB gateway's balance commands ('balancebegin', 'balanceget', 'balanceend',
'stepexbalance') refuse bad arguments with the gateway's error identifier before they look at the
handle, through the MEX API shim (tests/mex); the drop-in session names an op for each."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
PAR = np.tile(np.array([0.1, 0.01, 0.005]), (4, 1))


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_balance_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, a compensate that is not 0 / 1, an
    nsteps that is no count, params or a tc of the wrong class: all mpcekf:arg, and none
    dereferences the handle."""
    ok = {"balancebegin": (PAR, 1.0), "balanceget": (), "balanceend": (), "stepexbalance": (5.0,)}
    nout = {"balancebegin": 0, "balanceget": 1, "balanceend": 0, "stepexbalance": 9}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("balancebegin", "balanceend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: balanceget: at most 1 output"):
        shim.mex("balanceget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepexbalance: at most 9 outputs"):
        shim.mex("stepexbalance", DEAD, 5.0, nargout=10)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'balancebegin', h, params, compensate"):
        shim.mex("balancebegin", DEAD, PAR, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: balancebegin: params: expected ncells x 3 real doubles"):
        shim.mex("balancebegin", DEAD, np.zeros((4, 3), dtype=np.int32), 1.0, nargout=0)
    for bad in (2.0, -1.0, 0.5, float("nan")):
        with pytest.raises(shim.MexError, match="mpcekf:arg: balancebegin: compensate = .* is not 0 or 1"):
            shim.mex("balancebegin", DEAD, PAR, bad, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # 0 passes the checks
        shim.mex("balancebegin", DEAD, PAR, 0.0, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepexbalance', h, nsteps"):
        shim.mex("stepexbalance", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexbalance", DEAD, bad, nargout=0)
    with pytest.raises(shim.MexError,
                       match=r"mpcekf:arg: stepexbalance: tc: expected \[\] or ncells x nsteps real doubles"):
        shim.mex("stepexbalance", DEAD, 5.0, np.full((4, 5), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for tc passes the checks
        shim.mex("stepexbalance", DEAD, 0.0, np.zeros((0, 0)), nargout=9)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
    for call in ("mpcekf_balance_begin(h,", "mpcekf_balance_get(h,", "mpcekf_balance_end(h)",
                 "mpcekf_step_ex_balance(h,"):
        assert call in src, call


def test_the_output_array_holds_every_commands_outputs():
    """Every command builds its outputs in mexFunction's out[MAXOUT]: no command may promise more
    than MAXOUT outputs ('stepexbalance' has nine), and no gateway code may index past it."""
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    maxout = int(re.search(r"#define MAXOUT (\d+)", src).group(1))
    promised = [int(k) for k in re.findall(r"at most (\d+) outputs?", src)]
    assert promised and max(promised) == 9 and max(promised) <= maxout, (maxout, sorted(set(promised)))
    assert max(int(k) for k in re.findall(r"plhs\[(\d+)\]", src)) < maxout
    assert "mxArray *out[MAXOUT]" in src and "keep > MAXOUT" in src


def test_session_has_an_op_for_each_command():
    src = open(os.path.join(ROOT, "matlab", "dropin", "mpcekf_session.m")).read()
    for cmd in ("balancebegin", "balanceget", "balanceend", "stepexbalance"):
        assert f"case '{cmd}'" in src and f"mpcekf_mex('{cmd}', P.h" in src, cmd
