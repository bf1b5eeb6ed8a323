"""CPU: tests/obs_ref.ob_obs (the numpy restatement of OB_step's obs output) against the
existing oracle and against the identities of OB_step.m:289-356, and ROM.obs_layout().

ob_obs is the reference of tests/test_gpu_obs.py; here it is tied to oracle_np.ob_step:
driven side by side on 8 cells x 40 steps its Vcell is ob_step's bit for bit and its
pre-step averages are the oracle's state, in table mode and in handle mode.
"""
import numpy as np
import pytest

import obs_ref
from conftest import batch_inputs
import oracle_np as onp

N, STEPS = 8, 40


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("handles", [False, True], ids=["tables", "handles"])
@pytest.mark.parametrize("lookup", ["linear", "quintic"])
def test_ob_obs_rides_on_ob_step(P, lookup, handles):
    rom = P.make_synth_rom(lookup=lookup)
    soc0, tc = batch_inputs(N, seed=97)
    u = obs_ref.profile(rom, STEPS)
    for c in range(N):
        cs = onp.ob_step_init(rom, soc0[c], tc[c], handles=handles)
        for k in range(STEPS):
            pre_n, pre_p = cs["SOCnAvg"], cs["SOCpAvg"]
            o = obs_ref.ob_obs(rom, cs["bigX"].T, pre_n, pre_p, cs["SOC0n"], cs["SOC0p"], u[k], tc[c],
                               handles=handles)
            v = onp.ob_step(u[k], tc[c], cs)
            assert _bits(o["Vcell"]) == _bits(v), (c, k, o["Vcell"], v)
            assert _bits(o["negSOC"]) == _bits(pre_n) and _bits(o["posSOC"]) == _bits(pre_p)
            assert tuple(o) == obs_ref.OBS_FIELDS


def test_identities_and_field_lengths(rom):
    soc0, tc = batch_inputs(N, seed=101)
    u = obs_ref.profile(rom, STEPS)
    ind = onp.setup_inds(rom)
    cs = onp.ob_step_init(rom, soc0[0], tc[0])
    for k in range(STEPS):
        o, yk = obs_ref.ob_obs(rom, cs["bigX"].T, cs["SOCnAvg"], cs["SOCpAvg"], cs["SOC0n"], cs["SOC0p"], u[k],
                               tc[0], return_yk=True)
        onp.ob_step(u[k], tc[0], cs)
        assert _bits(o["Phie"][0]) == _bits(-o["negPhise0"])                       # OB_step.m:321
        assert o["Phie"].size == len(ind["Phie"]) + 1                              # OB_step.m:320
        np.testing.assert_array_equal(_bits(o["posPhis"]), _bits(yk[ind["posPhis"]] + o["Vcell"]))   # OB_step.m:348
        np.testing.assert_array_equal(_bits(o["Phie"][1:]), _bits(yk[ind["Phie"]] - o["negPhise0"]))
        for nm in ("negIfdl", "posIfdl", "negIf", "posIf", "negIdl", "posIdl", "negPhis", "posPhis", "negPhise",
                   "posPhise", "negThetass", "posThetass"):
            assert o[nm].shape == (len(ind[nm]),)
        assert o["Thetae"].shape == (len(ind["Thetae"]),)
        assert _bits(o["negThetass0"]) == _bits(o["negThetass"][0]) and _bits(o["negPhise0"]) == _bits(o["negPhise"][0])


def test_clamps_hold_out_of_range_and_nan(rom):
    """OB_step.m:307-310, 326 on a state pushed out of range: thetass inside [1e-6, 1 - 1e-6],
    thetae >= 1e-6, and a NaN entry clamps to 1e-6 (MATLAB's max ignores NaN)."""
    soc0, tc = batch_inputs(1, seed=103)
    cs = onp.ob_step_init(rom, soc0[0], tc[0])
    ind = onp.setup_inds(rom)
    th_rows = ind["negThetass"] + ind["posThetass"] + ind["Thetae"]
    for big in (1e6, -1e6, float("nan")):
        X = np.zeros((rom.NM, 6))
        X[:, 2:5] = big                       # the modes the thetass / thetae rows read
        o = obs_ref.ob_obs(rom, X, cs["SOCnAvg"], cs["SOCpAvg"], cs["SOC0n"], cs["SOC0p"], -30.0, tc[0])
        th = np.concatenate([o["negThetass"], o["posThetass"], [o["negThetass0"], o["posThetass3"]]])
        assert th.size and np.all((th >= 1e-6) & (th <= 1 - 1e-6)), (big, th)
        assert np.all(o["Thetae"] >= 1e-6), (big, o["Thetae"])
        if big != big:
            assert np.all(th == 1e-6) and np.all(o["Thetae"] == 1e-6)
    assert th_rows


def test_obs_layout_on_the_synthetic_rom(P, rom):
    lay = rom.obs_layout()
    assert tuple(lay) == obs_ref.OBS_FIELDS == P.rom.OBS_FIELDS            # the enum's order
    pos = 0
    for k, sl in lay.items():
        assert sl.start == pos and sl.stop >= sl.start and sl.step is None
        pos = sl.stop
    nobs = lay["Vcell"].stop
    assert sum(sl.stop - sl.start for sl in lay.values()) == nobs == 38
    ind = onp.setup_inds(rom)
    soc0, tc = batch_inputs(1, seed=107)
    cs = onp.ob_step_init(rom, soc0[0], tc[0])
    o = obs_ref.ob_obs(rom, cs["bigX"].T, cs["SOCnAvg"], cs["SOCpAvg"], cs["SOC0n"], cs["SOC0p"], -10.0, tc[0])
    for k, sl in lay.items():                                              # lengths agree with the reference's
        assert sl.stop - sl.start == np.atleast_1d(o[k]).size, k
    assert lay["Phie"].stop - lay["Phie"].start == len(ind["Phie"]) + 1


def test_obs_layout_zero_length_field(P, rom):
    """A ROM without posPhise rows: the field is there, zero slots long (OB_step.m:316 on an
    empty index), and every later field moves up."""
    import copy
    keep = [i for i, nm in enumerate(rom.names) if nm != "posPhise"]
    r2 = copy.copy(rom)
    r2.C, r2.D = rom.C[:, :, keep, :], rom.D[:, :, keep]
    r2.names, r2.xloc = [rom.names[i] for i in keep], np.asarray(rom.xloc)[keep]
    r2.validate()
    lay, full = r2.obs_layout(), rom.obs_layout()
    assert lay["posPhise"].start == lay["posPhise"].stop == full["posPhise"].start
    assert lay["Vcell"].stop == full["Vcell"].stop - 1
    soc0, tc = batch_inputs(1, seed=109)
    cs = onp.ob_step_init(r2, soc0[0], tc[0])
    o = obs_ref.ob_obs(r2, cs["bigX"].T, cs["SOCnAvg"], cs["SOCpAvg"], cs["SOC0n"], cs["SOC0p"], -10.0, tc[0])
    assert o["posPhise"].size == 0
