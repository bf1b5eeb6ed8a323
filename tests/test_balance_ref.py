"""CPU: tests/balance_ref.py, the header's passive-balancing rule in plain Python, on hand-written
cases for every branch (hysteresis on / hold / off, compensate 0 / 1, the u < 0 guard, NaN u or
z, an all-NaN string, ties in z and in e, -0.0 / +0.0, i_bleed = 0, S = 1, accumulation across
calls) and, with no bleeder, against tests/pack_ref.py on random commands."""
import numpy as np
import pytest

import balance_ref as br
import pack_ref as pr

NaN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        ok = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    else:
        ok = a == b
    assert ok.all(), (what, a, b)


def run(u, z, S, ib, on=0.01, off=0.005, comp=1, state=None):
    u, z = np.atleast_2d(np.asarray(u, float)), np.atleast_2d(np.asarray(z, float))
    return br.step(u, z, S, ib, on, off, comp, state=state)


def test_hysteresis_on_hold_off():
    # cell 1 against cell 0 (zmin = 0.5): d = 0.02 on, 0.008 held on, 0.004 off, 0.008 held off, 0.01 on (>=)
    z = np.array([[0.5, 0.52], [0.5, 0.508], [0.5, 0.504], [0.5, 0.508], [0.5, 0.51]])
    u = np.full((5, 2), -2.0)
    r = run(u, z, 2, 0.5, comp=0)
    same(r["bleed"], [[0, 0.5], [0, 0.5], [0, 0], [0, 0], [0, 0.5]], "bleed")
    same(r["u"], [[-2, -1.5], [-2, -1.5], [-2, -2], [-2, -2], [-2, -1.5]], "u")
    same(r["zmin"], np.full((5, 1), 0.5), "zmin")
    assert (r["limiter"] == 0).all()
    same(r["steps_on"], [0, 3]); same(r["q_bleed"], [0, 1.5]); same(r["switches"], [0, 2])
    same(r["bsteps"], [5, 5]); same(r["dz_max"], [0.0, 0.52 - 0.5]); same(r["dz_last"], [0.0, 0.51 - 0.5])
    same(r["on"], [0, 1])
    same(r["headroom"], [0, 0]); same(r["nlim"], [5, 0]); same(r["steps"], [5, 5])


def test_compensate_moves_the_limiter_and_the_guard_holds():
    # compensate = 0: e = u, limiter the largest u (cell 0), the bleeding cell 1 gets m + b
    z = [0.5, 0.6, 0.5]
    u = [-1.0, -1.2, -3.0]
    r = run(u, z, 3, [0.0, 0.5, 0.0], comp=0)
    same(r["e"], [u]); assert r["limiter"][0, 0] == 0
    same(r["u"], [[-1.0, -1.0 + 0.5, -1.0]])
    same(r["headroom"], [0.0, -1.0 - -1.2, 2.0])
    # compensate = 1: e_1 = -1.2 - 0.5 = -1.7; limiter still cell 0.  With u_0 = -2: e = (-2, -1.7, -3), limiter 1
    r = run([-2.0, -1.2, -3.0], z, 3, [0.0, 0.5, 0.0], comp=1)
    same(r["e"], [[-2.0, -1.2 - 0.5, -3.0]]); assert r["limiter"][0, 0] == 1
    m = -1.2 - 0.5
    same(r["u"], [[m, m + 0.5, m]])
    same(r["nlim"], [0, 1, 0]); same(r["headroom"], [m - -2.0, 0.0, m - -3.0])
    assert pr.reduce(np.array([[-2.0, -1.2, -3.0]]), 3)["limiter"][0, 0] == 1   # here the pack's limiter too
    r = run([-1.5, -1.2, -3.0], z, 3, [0.0, 0.5, 0.0], comp=1)     # e = (-1.5, -1.7, -3): limiter 0, the pack's 1
    assert r["limiter"][0, 0] == 0 and pr.reduce(np.array([[-1.5, -1.2, -3.0]]), 3)["limiter"][0, 0] == 1
    # the guard: a resting cell (+0.0) that bleeds is not compensated and still stops its string
    for zero in (0.0, -0.0):
        r = run([-2.0, zero, -3.0], z, 3, [0.0, 0.5, 0.0], comp=1)
        same(r["e"], [[-2.0, zero, -3.0]]); assert r["limiter"][0, 0] == 1
        same(r["u"], [[zero, zero + 0.5, zero]])
    # a discharging command (u > 0) is not compensated either
    r = run([-2.0, 0.3, -3.0], z, 3, [0.0, 0.5, 0.0], comp=1)
    same(r["e"], [[-2.0, 0.3, -3.0]]); same(r["u"], [[0.3, 0.8, 0.3]])


def test_nan_cells_and_all_nan_string():
    # string 0: cell 1 has a NaN command, cell 2 a NaN soc (a command, not valid); string 1: all NaN commands
    u = [-1.0, NaN, -0.5, -2.0, NaN, NaN, NaN, NaN]
    z = [0.7, 0.1, NaN, 0.5, 0.2, NaN, 0.3, 0.4]
    st = br.reset(8)
    st["on"][:] = 1                                   # flags left on by earlier steps
    r = run(u, z, 4, 0.25, comp=1, state=st)
    same(r["zmin"], [[0.5, NaN]])                     # cell 1 (0.1) is not valid: its command is NaN
    assert list(r["limiter"][0]) == [2, -1]           # e = (-1.25, -, -0.5, -2): the not-valid cell 2 is the limiter
    same(r["bleed"], [[0.25, NaN, 0.0, 0.0, NaN, NaN, NaN, NaN]])
    same(r["u"], [[-0.5 + 0.25, NaN, -0.5, -0.5, NaN, NaN, NaN, NaN]])
    same(r["on"], [1, 0, 0, 0, 0, 0, 0, 0])
    same(r["bsteps"], [1, 0, 0, 1, 0, 0, 0, 0]); same(r["steps"], [1, 0, 1, 1, 0, 0, 0, 0])
    same(r["dz_last"], [0.7 - 0.5, NaN, NaN, 0.0, NaN, NaN, NaN, NaN])
    same(r["dz_max"], [0.7 - 0.5, NaN, NaN, 0.0, NaN, NaN, NaN, NaN])
    same(r["switches"], np.zeros(8))                  # on -> on is no transition
    same(r["steps_on"], [1, 0, 0, 0, 0, 0, 0, 0])


def test_ties_and_signed_zeros():
    # a tie in z goes to the lowest index, and zmin has that cell's bits: -0.0 first, then +0.0
    r = run([-1.0, -1.0, -1.0], [0.0, -0.0, 0.0], 3, 0.5)
    same(r["zmin"], [[0.0]]); same(r["dz_last"], [0.0, -0.0 - 0.0, 0.0])
    r = run([-1.0, -1.0, -1.0], [-0.0, 0.0, 0.0], 3, 0.5)
    same(r["zmin"], [[-0.0]]); same(r["dz_last"], [-0.0 - -0.0, 0.0, 0.0])
    # a tie in e goes to the lowest index: cell 1's e = -1.5 - 0.5 equals cell 2's -2.0
    r = run([-3.0, -1.5, -2.0], [0.5, 0.6, 0.5], 3, [0.0, 0.5, 0.0], comp=1)
    same(r["e"], [[-3.0, -2.0, -2.0]]); assert r["limiter"][0, 0] == 1
    same(r["u"], [[-2.0, -1.5, -2.0]])
    # -0.0 == +0.0 by value among the commands: the lower index wins and its bits are applied
    r = run([-0.0, 0.0], [0.5, 0.5], 2, 0.5)
    assert r["limiter"][0, 0] == 0
    same(r["u"], [[-0.0, -0.0]])
    r = run([0.0, -0.0], [0.5, 0.5], 2, 0.5)
    same(r["u"], [[0.0, 0.0]])


def test_no_bleeder_and_series_one():
    # i_bleed = 0: the flag switches, nothing bleeds
    r = run([-1.0, -2.0], [0.5, 0.9], 2, 0.0)
    same(r["on"], [0, 1]); same(r["switches"], [0, 1]); same(r["steps_on"], [0, 0]); same(r["bleed"], [[0.0, 0.0]])
    same(r["u"], [[-1.0, -1.0]])
    # S = 1: d = 0 < dz_on, so even a flag left on goes off (0 <= dz_off) and u keeps its bits
    st = br.reset(3)
    st["on"][:] = 1
    u = np.array([[-1.0, -0.0, NaN]])
    r = run(u, [[0.2, 0.9, 0.5]], 1, 5.0, state=st)
    same(r["u"], u); same(r["on"], [0, 0, 0]); assert list(r["limiter"][0]) == [0, 0, -1]
    same(r["zmin"], [[0.2, 0.9, NaN]]); same(r["bleed"], [[0.0, 0.0, NaN]])
    same(r["nlim"], [1, 1, 0]); same(r["headroom"], [0, 0, 0])


def test_accumulation_across_calls_through_state():
    rng = np.random.Generator(np.random.PCG64(0xBA1A))
    n, S, N = 24, 6, 30
    u = -rng.uniform(0.5, 3.0, (N, n))
    z = rng.uniform(0.4, 0.45, (N, n))
    u[rng.random((N, n)) < 0.05] = NaN
    z[rng.random((N, n)) < 0.05] = NaN
    ib = rng.choice([0.0, 0.3, 1.0], n)
    one = br.step(u, z, S, ib, 0.02, 0.01, 1)
    st, parts = None, []
    for a, b in ((0, 7), (7, 8), (8, 30)):
        st = br.step(u[a:b], z[a:b], S, ib, 0.02, 0.01, 1, state=st)
        parts.append(st)
    for k in ("u", "bleed", "zmin", "limiter", "e"):
        same(np.concatenate([p[k] for p in parts]), one[k], k)
    for k in br.PACK_FIELDS + br.FIELDS + ("on",):
        same(parts[-1][k], one[k], k)
    assert one["switches"].max() >= 2 and one["steps_on"].sum() > 0 and (one["bsteps"] < N).any()


@pytest.mark.parametrize("S", [1, 2, 7, 64])
def test_without_a_bleeder_it_is_the_pack_rule(S):
    rng = np.random.Generator(np.random.PCG64(S))
    n, N = S * 5, 12
    u = rng.choice(np.array([-3.0, -1.0, -0.0, 0.0, 0.5, NaN]), (N, n)) * rng.choice([1.0, 1.0, 2.0], (N, n))
    z = rng.uniform(0.1, 0.9, (N, n))
    z[rng.random((N, n)) < 0.1] = NaN
    want = pr.reduce(u, S)
    for comp in (0, 1):
        got = br.step(u, z, S, 0.0, 0.01, 0.005, comp)
        for k in ("u", "limiter") + pr.FIELDS:
            same(got[k], want[k], f"i_bleed = 0: {k}")
        same(got["steps_on"], np.zeros(n)); same(got["q_bleed"], np.zeros(n))
        # and a dz_on that no cell reaches
        got = br.step(u, z, S, 1.0, 5.0, 0.0, comp)
        for k in ("u", "limiter") + pr.FIELDS:
            same(got[k], want[k], f"unreachable dz_on: {k}")


def test_bad_arguments():
    with pytest.raises(ValueError, match="series = 4"):
        br.step(np.zeros((1, 6)), np.zeros((1, 6)), 4, 0.0, 0.01, 0.0, 1)
    with pytest.raises(ValueError, match="compensate = 2"):
        br.step(np.zeros((1, 6)), np.zeros((1, 6)), 3, 0.0, 0.01, 0.0, 2)
