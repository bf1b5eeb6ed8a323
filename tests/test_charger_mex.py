"""CPU: the MATLAB gateway's charger commands ('chargerbegin', 'chargerget', 'chargerend',
'stepexcharger') refuse bad arguments with the gateway's error identifier before they look at the
handle, through the MEX API shim (tests/mex); the drop-in session names an op for each and keeps
an optional `charger` field."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
PAR = np.tile(np.array([20.0, 700.0]), (4, 1))


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_charger_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, an nsteps that is no count, params
    or a tc of the wrong class: all mpcekf:arg, and none dereferences the handle."""
    ok = {"chargerbegin": (PAR,), "chargerget": (), "chargerend": (), "stepexcharger": (5.0,)}
    nout = {"chargerbegin": 0, "chargerget": 1, "chargerend": 0, "stepexcharger": 9}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("chargerbegin", "chargerend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: chargerget: at most 1 output"):
        shim.mex("chargerget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepexcharger: at most 9 outputs"):
        shim.mex("stepexcharger", DEAD, 5.0, nargout=10)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'chargerbegin', h, params"):
        shim.mex("chargerbegin", DEAD, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: chargerbegin: params: expected nstrings x 2 real doubles"):
        shim.mex("chargerbegin", DEAD, np.zeros((4, 2), dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepexcharger', h, nsteps"):
        shim.mex("stepexcharger", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexcharger", DEAD, bad, nargout=0)
    with pytest.raises(shim.MexError,
                       match=r"mpcekf:arg: stepexcharger: tc: expected \[\] or ncells x nsteps real doubles"):
        shim.mex("stepexcharger", DEAD, 5.0, np.full((4, 5), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for tc passes the checks
        shim.mex("stepexcharger", DEAD, 0.0, np.zeros((0, 0)), nargout=9)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
    for call in ("mpcekf_charger_begin(h,", "mpcekf_charger_get(h,", "mpcekf_charger_end(h)",
                 "mpcekf_step_ex_charger(h,"):
        assert call in src, call


def test_no_existing_command_changes_its_output_count():
    """'stepexcharger' carries its five extra rows in two structs, so the gateway's output array
    and every existing command's promise stay what they were."""
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    assert re.search(r"#define MAXOUT 9\b", src)
    assert "stepexbalance: at most 9 outputs [u, v, soc, phise, nexec, ucmd, limiter, bleed, zmin]" in src
    assert "stepexcharger: at most 9 outputs [u, v, soc, phise, nexec, ucmd, limiter, bal, chg]" in src


def test_session_has_an_op_for_each_command_and_a_charger_field():
    src = open(os.path.join(ROOT, "matlab", "dropin", "mpcekf_session.m")).read()
    for cmd in ("chargerbegin", "chargerget", "chargerend", "stepexcharger"):
        assert f"case '{cmd}'" in src and f"mpcekf_mex('{cmd}', P.h" in src, cmd
    assert "'charger', []" in src and "name = P.charger" in src and "P.charger = name" in src
