"""GPU: OB_step's obs output end to end (mpcekf_plant_step_obs / mpcekf_plant_obs_slots,
Context.OB_step(obs=...), the gateway's 'plantobs').

Reference: tests/obs_ref.ob_obs in table mode on the state read back before each step
(get_state), tolerance 1e-12 * max(1, max|field|) -- the project's C-vs-numpy bound.
Shapes n = 1, 3, 65, 257: a partial quad / wave, a wave boundary (16 cells a wave), a block
boundary of the quad-per-cell kernel.  Everything that exists today must keep its bits.
"""
import copy
import os

import numpy as np
import pytest

import mexshim
import obs_ref
from conftest import ROOT, batch_inputs

pytestmark = pytest.mark.gpu

STEPS = 12
SCALARS = ("negSOC", "posSOC", "cellSOC", "negIfdl0", "posIfdl3", "negIf0", "posIf3", "negThetass0", "posThetass3",
           "negPhise0", "Vcell")


@pytest.fixture(scope="module")
def M(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.mpcekf")


@pytest.fixture(scope="module")
def R(P):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd.rom")


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ in bits"


def _ref_step(rom, st, soc0n, soc0p, u, tc):
    """ob_obs on every cell of a get_state() snapshot: {field: [n] or [n, len]}."""
    n = st["scal"].shape[0]
    per = [obs_ref.ob_obs(rom, st["bigX"][c], st["scal"][c, 0], st["scal"][c, 1], soc0n[c], soc0p[c], u[c], tc[c])
           for c in range(n)]
    return {k: np.array([p[k] for p in per]).reshape((n,) if k in SCALARS else (n, -1)) for k in obs_ref.OBS_FIELDS}


def _check_against_ref(M, rom, n, seed, steps=STEPS, tol=1e-12):
    soc0, tc = batch_inputs(n, seed=seed)
    u = obs_ref.profile(rom, steps)
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        st0 = ctx.get_state()
        soc0n, soc0p = st0["scal"][:, 0].copy(), st0["scal"][:, 1].copy()   # SOC0n/p: the initial averages
        assert ctx.obs_layout() == rom.obs_layout()
        for k in range(steps):
            st = ctx.get_state()
            uk = np.full(n, u[k])
            v, o = ctx.OB_step(uk, obs=True)
            ref = _ref_step(rom, st, soc0n, soc0p, uk, tc)
            assert tuple(o) == obs_ref.OBS_FIELDS
            _bits_equal(o["Vcell"], v, f"step {k} obs.Vcell vs V")
            for f in obs_ref.OBS_FIELDS:
                assert o[f].shape == ref[f].shape, (f, o[f].shape, ref[f].shape)
                if not ref[f].size:
                    continue
                err = float(np.max(np.abs(o[f] - ref[f])))
                atol = tol * max(1.0, float(np.max(np.abs(ref[f]))))
                print(f"n={n} step {k} {f}: max err {err:.3g} (atol {atol:.3g})")
                assert err <= atol, (f, k, err, atol)


@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("lookup", ["linear", "quintic"])
def test_obs_matches_reference(P, M, lookup, n):
    _check_against_ref(M, P.make_synth_rom(lookup=lookup), n, seed=127 + n)


@pytest.mark.parametrize("n", [3, 65])
def test_obs_matches_reference_node_tables(M, R, n):
    _check_against_ref(M, R.make_tab_rom("linear", T_eval_degC=(25.0,)), n, seed=131 + n)


def test_existing_plant_step_keeps_its_bits(P, M):
    rom = P.make_synth_rom(lookup="quintic")
    n = 257
    soc0, tc = batch_inputs(n, seed=137)
    u = obs_ref.profile(rom, STEPS)
    with M.Context(rom, n) as a, M.Context(rom, n) as b:
        a.init_cells(soc0, tc)
        b.init_cells(soc0, tc)
        for k in range(STEPS):
            uk = np.full(n, u[k])
            va = a.OB_step(uk)
            vb, o = b.OB_step(uk, obs=True)
            _bits_equal(va, vb, f"V step {k}")
            _bits_equal(o["Vcell"], va, f"obs.Vcell step {k}")
        sa, sb = a.get_state(), b.get_state()
        for key in ("bigX", "scal"):
            _bits_equal(sa[key], sb[key], f"state {key}")


def test_stage_route_closed_loop_with_obs_call(P, M):
    """test_gpu_stage_route's device route with the plant call replaced by the obs call: u is
    the fused runMPC command at every step, bit for bit."""
    rom = P.make_synth_rom()
    n, steps = 96, 20
    soc0, tc = batch_inputs(n, seed=83)
    fused = M.runMPC(rom, soc0, tc, steps)
    with M.Context(rom, n) as dev:
        dev.init_cells(soc0, tc)
        ud = np.zeros(n)
        for k in range(steps):
            vd, o = dev.OB_step(ud, obs=("negPhise0",))
            zd, _, _ = dev.iterEKF(vd, ud, xind=False)
            assert dev.EKFmatsHandler(None, None, keep=True) is None
            ud, _ = dev.iterMPC(None, zd[:, -1])
            _bits_equal(ud, fused["u"][k], f"u step {k}")
            _bits_equal(vd, fused["v"][k], f"v step {k}")
            assert o["negPhise0"].shape == (n,) and np.all(np.isfinite(o["negPhise0"]))


def _run_full(M, rom, n, seed, steps=4, status=None):
    soc0, tc = batch_inputs(n, seed=seed)
    u = obs_ref.profile(rom, steps)
    out = []
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        if status is not None:
            st = ctx.get_state()
            st["status"] = status
            ctx.set_state(st)
        for k in range(steps):
            out.append(ctx.OB_step(np.full(n, u[k]), obs=True))
    return out


def test_phise_res0_column_is_ignored(P, M):
    """OB_step.m:178-181: a ROM whose negPhise / posPhise rows carry a non-zero res0 column gives
    the obs of the ROM with zeros there, and still matches ob_obs (which zeroes it too)."""
    rom = P.make_synth_rom()
    dirty = copy.copy(rom)
    dirty.C = rom.C.copy()
    rows = [i for i, nm in enumerate(rom.names) if nm in ("negPhise", "posPhise")]
    dirty.C[:, :, rows, -1] = 0.37
    n = 65
    a, b = _run_full(M, rom, n, 139), _run_full(M, dirty, n, 139)
    for k, ((va, oa), (vb, ob)) in enumerate(zip(a, b)):
        _bits_equal(va, vb, f"V step {k}")
        for f in obs_ref.OBS_FIELDS:
            _bits_equal(oa[f], ob[f], f"{f} step {k}")
    _check_against_ref(M, dirty, 3, seed=139, steps=6)


@pytest.mark.parametrize("grid", ["one_T", "one_Z", "large_NM"])
def test_duplicate_corners_and_rom_global(P, M, grid):
    """A single-temperature and a single-SOC ROM (duplicate corners), and the NM = 147 ROM of
    tests/test_gpu_rom_size.py whose model rows do not fit the LDS (rom_global), n = 65."""
    if grid == "one_T":
        rom = P.make_synth_rom(T_degC=(25.0,))
    elif grid == "one_Z":
        rom = P.make_synth_rom(SOC_pct=(50.0,))
    else:
        rom = P.make_synth_rom(T_degC=tuple(np.linspace(15.0, 35.0, 7)), SOC_pct=tuple(np.linspace(0.0, 100.0, 21)))
        assert rom.NM == 147
    _check_against_ref(M, rom, 65, seed=149, steps=6)


def test_slots_subset_async_and_state_errors(P, M):
    rom = P.make_synth_rom(lookup="quintic")
    n = 65
    soc0, tc = batch_inputs(n, seed=151)
    u = np.full(n, -20.0)
    lay = rom.obs_layout()
    with M.Context(rom, n) as full, M.Context(rom, n) as part, M.Context(rom, n) as asy:
        for c in (full, part, asy):
            c.init_cells(soc0, tc)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5.*no mpcekf_plant_step_obs"):   # before any obs call
            part.plant_obs_slots([0])
        asy.asynchronous = True
        for k in range(3):
            vf, of = full.OB_step(u, obs=True)
            vp, op = part.OB_step(u, obs=("negPhise0", "Thetae"))
            va, oa = asy.OB_step(u, obs=True)
            asy.sync()
            assert tuple(op) == ("negPhise0", "Thetae") and op["Thetae"].shape == (n, 3)
            _bits_equal(vp, vf, "V")
            for f in op:
                _bits_equal(op[f], of[f], f"subset {f} step {k}")
            _bits_equal(va, vf, "async V")
            for f in of:
                _bits_equal(oa[f], of[f], f"async {f} step {k}")
        sl = [lay["Vcell"].start, lay["Phie"].start]
        rows = part.plant_obs_slots(sl)
        _bits_equal(rows[0], of["Vcell"], "slot Vcell")
        _bits_equal(rows[1], of["Phie"][:, 0], "slot Phie(1)")
        for bad in (-1, lay["Vcell"].stop):
            with pytest.raises(M.MpcekfError, match="mpcekf error -1"):
                part.plant_obs_slots([bad])
        part.step(1)
        with pytest.raises(M.MpcekfError, match="mpcekf error -5"):                             # after a fused step
            part.plant_obs_slots(sl)
        part.OB_step(u, obs=())
        part.plant_obs_slots(sl)
        part.set_state(part.get_state())
        with pytest.raises(M.MpcekfError, match="mpcekf error -5"):                             # after set_state
            part.plant_obs_slots(sl)


def test_error_cell_is_nan_and_neighbours_unaffected(P, M, R):
    rom = P.make_synth_rom()
    n, bad = 65, 17
    status = np.zeros(n, dtype=np.int32)
    clean = _run_full(M, rom, n, 157, status=status)
    status[bad] = 1                                                     # MPCEKF_ST_ERROR
    err = _run_full(M, rom, n, 157, status=status)
    keep = np.arange(n) != bad
    for k, ((vc, oc_), (ve, oe)) in enumerate(zip(clean, err)):
        assert np.isnan(ve[bad])
        _bits_equal(ve[keep], vc[keep], f"V step {k}")
        for f in obs_ref.OBS_FIELDS:
            assert np.all(np.isnan(oe[f][bad])), (f, k)
            _bits_equal(oe[f][keep], oc_[f][keep], f"{f} step {k}")


def test_fixture_handle_mode_quintic(P, M):
    """tests/golden/obs_batch8_40.npz (handle mode, tools/make_obs_golden.py) against the quintic
    ROM's tables: the README's handle-parity bound, 1e-6 relative to max(1, |field|)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "obs_batch8_40.npz"))
    rom = P.make_synth_rom(lookup="quintic")
    soc0, tc, u = g["soc0"], g["tc"], g["u"]
    n = soc0.size
    with M.Context(rom, n) as ctx:
        ctx.init_cells(soc0, tc)
        for k in range(u.size):
            _, o = ctx.OB_step(np.full(n, u[k]), obs=True)
            for f in obs_ref.OBS_FIELDS:
                ref = g["obs_" + f][k]
                got = o[f].reshape(ref.shape)
                if ref.size:
                    e = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
                    assert e <= 1e-6, (f, k, e)


def test_plantobs_through_gateway(P, M):
    mexshim.build()
    rom = P.make_synth_rom()
    n, steps = 96, 5
    soc0, tc = batch_inputs(n, seed=163)
    u = obs_ref.profile(rom, steps)
    h = mexshim.mex("create", mexshim.rom_struct(rom), {}, 0.0, float(n))
    try:
        with M.Context(rom, n) as ctx:
            mexshim.mex("init", h, soc0, tc, nargout=0)
            ctx.init_cells(soc0, tc)
            off = mexshim.mex("obslayout", h)
            assert [int(x) for x in off.ravel()] == [s.start for s in rom.obs_layout().values()] + [38]
            for k in range(steps):
                uk = np.full(n, u[k])
                v_m, o_m = mexshim.mex("plantobs", h, uk, tc, nargout=2)
                v_c, o_c = ctx.OB_step(uk, tc, obs=True)
                _bits_equal(v_m, v_c[None, :], f"V step {k}")
                assert list(o_m) == list(obs_ref.OBS_FIELDS)
                for f in obs_ref.OBS_FIELDS:                         # MATLAB: len x ncells
                    _bits_equal(o_m[f], np.atleast_2d(o_c[f].T), f"{f} step {k}")
            rows = mexshim.mex("obsslots", h, np.array([[38.0, 1.0]]))
            _bits_equal(rows, np.stack([o_c["Vcell"], o_c["negSOC"]]), "obsslots")
            with pytest.raises(mexshim.MexError, match="mpcekf:arg: obsslots: idx.* is not a slot 1..38"):
                mexshim.mex("obsslots", h, np.array([[39.0]]))
            with pytest.raises(mexshim.MexError, match="mpcekf:arg: iapp: expected 96 real doubles"):
                mexshim.mex("plantobs", h, np.zeros(95), tc, nargout=2)
    finally:
        mexshim.mex("destroy", h, nargout=0)
