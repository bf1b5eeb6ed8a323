"""GPU: the MATLAB gateway's charger commands on a live context, through the MEX API shim: the
nine outputs of 'stepexcharger' are all delivered and equal the ctypes path's bits, with and
without a balancer; 'chargerget' returns the record, 'chargerend' ends the charger."""
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


@pytest.mark.parametrize("balanced", [False, True])
def test_stepexcharger_delivers_nine_outputs(shim, rom, M, balanced):
    n, S, N = 48, 12, 12
    soc0, tc, lim, par = tb.inputs(n, S)
    chg = (np.array([20.0, np.nan, 40.0, 25.0]), np.array([np.nan, 700.0, 600.0, np.inf]))
    names = ("u", "v", "soc", "phise", "nexec", "ucmd", "limiter")
    h = shim.mex("create", shim.rom_struct(rom), {}, 0.0, float(n))
    try:
        shim.mex("init", h, soc0, tc, nargout=0)
        with pytest.raises(shim.MexError, match="mpcekf error -5: charger_begin"):         # no pack yet
            shim.mex("chargerbegin", h, np.full((n, 2), 20.0), nargout=0)
        shim.mex("packbegin", h, float(S), nargout=0)
        if balanced:
            shim.mex("balancebegin", h, np.ascontiguousarray(np.stack(par).T), 1.0, nargout=0)
        with pytest.raises(shim.MexError, match="mpcekf error -5: step_ex_charger"):       # no charger yet
            shim.mex("stepexcharger", h, 1.0, nargout=9)
        with pytest.raises(shim.MexError, match="mpcekf:arg: chargerbegin: params"):       # ncells x 2 is the wrong size
            shim.mex("chargerbegin", h, np.full((n, 2), 20.0), nargout=0)
        shim.mex("chargerbegin", h, np.ascontiguousarray(np.stack(chg).T), nargout=0)      # nstrings x 2
        outs = shim.mex("stepexcharger", h, float(N), nargout=9)
        with pytest.raises(shim.MexError, match="mpcekf:arg: stepexcharger: at most 9 outputs"):
            shim.mex("stepexcharger", h, 1.0, nargout=10)
        chg_only = shim.mex("stepexcharger", h, 2.0, nargout=9)[8]
        rec = shim.mex("chargerget", h)
        shim.mex("chargerend", h, nargout=0)
        with pytest.raises(shim.MexError, match="mpcekf error -5: charger_get"):
            shim.mex("chargerget", h)
    finally:
        shim.mex("destroy", h, nargout=0)
    rows = ("ucmd", "limiter", "vstr", "istr", "capby") + (("bleed", "zmin") if balanced else ())
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        ctx.pack_begin(S)
        if balanced:
            ctx.balance_begin(*par)
        ctx.charger_begin(*chg)
        ref = ctx.step(N, outputs=names[:5], pack=rows)
        more = ctx.step(2, outputs=(), pack=("istr",))
        want = ctx.charger_get()
    assert len(outs) == 9 and all(o is not None for o in outs)
    for k, a in zip(names, outs[:7]):
        assert a.shape == ((n // S if k == "limiter" else n), N), k                        # MATLAB: rows x nsteps
        same(np.ascontiguousarray(a.T), ref[k] + 1 if k == "limiter" else ref[k], f"gateway: {k}")   # limiter 1-based
    bal, ch = outs[7], outs[8]
    assert sorted(bal) == ["bleed", "zmin"] and sorted(ch) == ["capby", "istr", "vstr"]
    for k in ("vstr", "istr", "capby"):
        assert ch[k].shape == (n // S, N), k
        same(np.ascontiguousarray(ch[k].T), ref[k], f"gateway: {k}")
    if balanced:
        for k in ("bleed", "zmin"):
            same(np.ascontiguousarray(bal[k].T), ref[k], f"gateway: {k}")
    else:
        assert bal["bleed"].size == 0 and bal["zmin"].size == 0
    same(np.ascontiguousarray(chg_only["istr"].T), more["istr"], "gateway: istr of a second call")
    assert (ch["capby"] == 1).any() and (ch["capby"] == 2).any() and (outs[6] == -1).any()   # a capped step's limiter
    for k, v in want.items():
        same(np.ascontiguousarray(rec[k].ravel()), v, f"gateway: charger record {k}")
