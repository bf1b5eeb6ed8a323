"""GPU: the MATLAB gateway's balance commands on a live context, through the MEX API shim: the
nine outputs of 'stepexbalance' are all delivered and equal the ctypes path's bits, 'balanceget'
returns the record, 'balanceend' ends the balancer."""
import numpy as np
import pytest

import mexshim
import test_gpu_balance as tb
from test_gpu_pack import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_stepexbalance_delivers_nine_outputs(shim, rom, M):
    n, S, N = 48, 12, 12
    soc0, tc, lim, par = tb.inputs(n, S)
    names = ("u", "v", "soc", "phise", "nexec", "ucmd", "limiter", "bleed", "zmin")
    h = shim.mex("create", shim.rom_struct(rom), {}, 0.0, float(n))
    try:
        shim.mex("init", h, soc0, tc, nargout=0)
        shim.mex("packbegin", h, float(S), nargout=0)
        shim.mex("balancebegin", h, np.ascontiguousarray(np.stack(par).T), 1.0, nargout=0)   # ncells x 3
        outs = shim.mex("stepexbalance", h, float(N), nargout=9)
        with pytest.raises(shim.MexError, match="mpcekf:arg: stepexbalance: at most 9 outputs"):
            shim.mex("stepexbalance", h, 1.0, nargout=10)
        zmin_only = shim.mex("stepexbalance", h, 2.0, nargout=9)[8]
        rec = shim.mex("balanceget", h)
        shim.mex("balanceend", h, nargout=0)
        with pytest.raises(shim.MexError, match="mpcekf error -5: balance_get"):
            shim.mex("balanceget", h)
    finally:
        shim.mex("destroy", h, nargout=0)
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.pack_begin(S)
        ctx.balance_begin(*par)
        ref = ctx.step(N, outputs=names[:5], pack=names[5:])
        more = ctx.step(2, outputs=(), pack=("zmin",))
        want = ctx.balance_get()
    assert len(outs) == 9 and all(o is not None for o in outs)
    for k, a in zip(names, outs):
        assert a.shape == ((n // S if k in ("limiter", "zmin") else n), N), k       # MATLAB: rows x nsteps
        same(np.ascontiguousarray(a.T), ref[k] + 1 if k == "limiter" else ref[k], f"gateway: {k}")   # limiter 1-based
    same(np.ascontiguousarray(zmin_only.T), more["zmin"], "gateway: zmin of a second call")
    assert (outs[7] > 0).any() and np.isfinite(outs[8]).all()
    for k, v in want.items():
        same(np.ascontiguousarray(rec[k].ravel()), v, f"gateway: balance record {k}")
