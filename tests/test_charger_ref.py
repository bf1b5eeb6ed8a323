"""CPU: tests/charger_ref.py, the plain-Python restatement of the charger rule of
include/mpcekf.h (mpcekf_charger_begin), on cases written out by hand: the tree's shape, a term
of -0.0, NaN cells, the caps and their tie, a resting string, every record field, the
identities."""
import numpy as np
import pytest

import balance_ref as br
import charger_ref as cr
import pack_ref as pr

NAN = float("nan")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.dtype.kind == "f":
        assert (((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))).all(), (what, a, b)
    else:
        assert (a == b).all(), (what, a, b)


# ---- the tree -----------------------------------------------------------------------------------
def test_tree_written_out_by_hand():
    f = np.float64
    x = [f(0.1), f(0.7), f(1e-17), f(3.3), f(-2.9), f(1e16), f(0.3), f(5e-324)]
    assert bits(cr.tree_sum(x[:1])) == bits(x[0])
    assert bits(cr.tree_sum(x[:2])) == bits(x[0] + x[1])
    assert bits(cr.tree_sum(x[:3])) == bits((x[0] + x[1]) + x[2])
    assert bits(cr.tree_sum(x[:5])) == bits(((x[0] + x[1]) + (x[2] + x[3])) + x[4])
    assert bits(cr.tree_sum(x[:8])) == bits(((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])))
    # 6 and 7: a partner at or beyond S is skipped at every level
    assert bits(cr.tree_sum(x[:6])) == bits(((x[0] + x[1]) + (x[2] + x[3])) + (x[4] + x[5]))
    assert bits(cr.tree_sum(x[:7])) == bits(((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + x[6]))


def test_tree_is_not_the_sequential_sum():
    x = [1e16, 1.0, 1.0, 1.0]
    assert cr.tree_sum(x) == 1.0000000000000002e16       # (1e16 + 1) + (1 + 1) = 1e16 + 2
    seq = np.float64(0.0)
    for a in x:
        seq = seq + np.float64(a)
    assert seq == 1e16
    u = np.full(4, -1.0)
    V, nvalid = cr.string_voltage(u, x)
    assert V == 1.0000000000000002e16 and nvalid == 4


def test_negative_zero_and_nan_terms():
    V, nv = cr.string_voltage([-1.0], [-0.0])
    assert bits(V) == bits(0.0) and nv == 1              # v + 0.0: S = 1 gives +0.0, not -0.0
    V, nv = cr.string_voltage([-1.0, -1.0], [-0.0, -0.0])
    assert bits(V) == bits(0.0) and nv == 2
    # a NaN command or a NaN voltage: the term is +0.0 and the cell does not count
    V, nv = cr.string_voltage([-1.0, NAN, -1.0, -1.0, -2.0], [3.5, 3.6, NAN, 3.7, 3.25])
    assert bits(V) == bits(((3.5 + 0.0) + (0.0 + 3.7)) + 3.25) and nv == 3
    V, nv = cr.string_voltage([NAN, NAN], [3.5, 3.6])
    assert bits(V) == bits(0.0) and nv == 0


# ---- the caps -----------------------------------------------------------------------------------
def test_caps_by_hand():
    f = np.float64
    assert cr.caps(f(-30.0), f(40.0), NAN, NAN) == (-30.0, 0)
    assert cr.caps(f(-30.0), f(40.0), 20.0, NAN) == (-20.0, 1)
    assert cr.caps(f(-30.0), f(40.0), 30.0, NAN) == (-30.0, 0)           # cap == m: not capped
    assert cr.caps(f(-30.0), f(40.0), NAN, 1000.0) == (-25.0, 2)
    assert cr.caps(f(-30.0), f(40.0), 20.0, 1000.0) == (-20.0, 1)        # the larger of the two
    assert cr.caps(f(-30.0), f(40.0), 28.0, 1000.0) == (-25.0, 2)
    assert cr.caps(f(-30.0), f(40.0), 25.0, 1000.0) == (-25.0, 1)        # a tie: the current cap wins
    assert cr.caps(f(-30.0), f(40.0), np.inf, np.inf) == (-30.0, 0)      # +inf never binds
    assert cr.caps(f(-30.0), f(0.0), NAN, 1000.0) == (-30.0, 0)          # V_g > 0 or no power cap
    assert cr.caps(f(-30.0), f(-3.0), NAN, 1000.0) == (-30.0, 0)
    m, by = cr.caps(f(-30.0), f(3.0), NAN, 1.0)
    assert bits(m) == bits(-(f(1.0) / f(3.0))) and by == 2               # one rounded division
    m, by = cr.caps(f(-30.0), f(40.0), 0.0, NAN)
    assert bits(m) == bits(-0.0) and by == 1                             # m' = cap bit for bit
    # a resting string and a discharging one are never capped
    for rest in (f(0.0), f(-0.0), f(2.5)):
        m, by = cr.caps(rest, f(40.0), 0.0, 1e-9)
        assert bits(m) == bits(rest) and by == 0


# ---- the whole step -----------------------------------------------------------------------------
def test_step_rows_and_every_record_field():
    S = 3
    # string 0: capped by power, then by current, then loose; string 1: a NaN cell, then no command at all
    ucmd = np.array([[-30.0, -20.0, -25.0, -10.0, NAN, -12.0],
                     [-30.0, -20.0, -25.0, NAN, NAN, NAN],
                     [-5.0, -4.0, -6.0, 0.0, -3.0, -2.0]])
    v = np.array([[3.5, 3.6, 3.7, 3.0, 3.1, 3.2],
                  [3.6, 3.7, 3.8, 3.0, 3.1, 3.2],
                  [3.7, 3.8, 3.9, 3.3, NAN, 3.4]])
    soc = np.zeros_like(v)
    i_max, p_max = np.array([15.0, NAN]), np.array([108.0, 31.0])
    r = cr.step(ucmd, soc, v, S, i_max, p_max)
    f = np.float64
    V00 = (f(3.5) + f(3.6)) + f(3.7)
    V01 = (f(3.6) + f(3.7)) + f(3.8)
    V02 = (f(3.7) + f(3.8)) + f(3.9)
    V10 = f(3.0) + f(3.2)                                # (3.0 + 0.0) + 3.2
    V12 = (f(3.3) + f(0.0)) + f(3.4)
    same(r["vstr"], np.array([[V00, V10], [V01, 0.0], [V02, V12]]), "vstr")
    c00 = -(f(108.0) / V00)                              # -10: above -15, the power cap
    c01 = -(f(108.0) / V01)                              # -9.73
    c10 = -(f(31.0) / V10)                               # -5
    assert c00 > -15.0 and c01 > -15.0 and c10 > -10.0
    same(r["mraw"], np.array([[-20.0, -10.0], [-20.0, NAN], [-4.0, 0.0]]), "mraw")
    same(r["istr"], np.array([[c00, c10], [c01, NAN], [-4.0, 0.0]]), "istr")
    same(r["capby"], np.array([[2, 2], [2, -1], [0, 0]], dtype=np.int32), "capby")
    same(r["limiter"], np.array([[-2, -2], [-2, -1], [1, 0]], dtype=np.int32), "limiter")
    same(r["u"], np.array([[c00, c00, c00, c10, NAN, c10], [c01, c01, c01, NAN, NAN, NAN],
                           [-4.0, -4.0, -4.0, 0.0, 0.0, 0.0]]), "u")
    ch, pk = r["st"]["charger"], r["st"]["pack"]
    same(ch["steps"], [3.0, 2.0]); same(ch["ncap_i"], [0.0, 0.0]); same(ch["ncap_p"], [2.0, 1.0])
    same(ch["q"], [(f(0.0) + c00 + c01) + f(-4.0), (f(0.0) + c10) + f(0.0)])
    same(ch["e"], [((f(0.0) + V00 * c00) + V01 * c01) + V02 * f(-4.0), (f(0.0) + V10 * c10) + V12 * f(0.0)])
    same(ch["curtail"], [((f(0.0) + (c00 - f(-20.0))) + (c01 - f(-20.0))) + f(0.0), (f(0.0) + (c10 - f(-10.0))) + f(0.0)])
    same(ch["p_min"], [min(V00 * c00, V01 * c01, V02 * f(-4.0)), V10 * c10])
    same(ch["v_peak"], [V02, V12]); same(ch["nvalid_min"], [3.0, 2.0])
    same(pk["steps"], [3.0, 3.0, 3.0, 2.0, 1.0, 2.0])
    same(pk["nlim"], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0])    # NLIM counts nothing on a capped step
    same(pk["headroom"][:3], [(f(0.0) + (c00 + 30.0) + (c01 + 30.0)) + 1.0, (f(0.0) + (c00 + 20.0) + (c01 + 20.0)) + 0.0,
                              (f(0.0) + (c00 + 25.0) + (c01 + 25.0)) + 2.0])
    # the current cap: a second call goes on from the first one's state
    r2 = cr.step(ucmd[:1], soc[:1], v[:1], S, np.array([15.0, 4.0]), np.array([NAN, NAN]), state=r["st"])
    same(r2["istr"], [[-15.0, -4.0]]); same(r2["capby"], np.array([[1, 1]], dtype=np.int32))
    same(r2["st"]["charger"]["ncap_i"], [1.0, 1.0]); same(r2["st"]["charger"]["steps"], [4.0, 3.0])
    assert (r["st"]["charger"]["steps"] == [3.0, 2.0]).all()             # the earlier state is not changed in place


def test_with_a_balancer_the_cap_replaces_e_lim():
    S = 2
    ucmd = np.array([[-30.0, -20.0]])
    soc = np.array([[0.50, 0.40]])                        # cell 0 is 0.1 ahead: it bleeds 2 A
    v = np.array([[3.5, 3.25]])
    bal = (np.array([2.0, 2.0]), np.full(2, 0.01), np.full(2, 0.005), 1)
    free = cr.step(ucmd, soc, v, S, NAN, NAN, balance=bal)
    b = br.step(ucmd, soc, S, *bal)
    same(free["u"], b["u"]); same(free["limiter"], b["limiter"]); same(free["bleed"], b["bleed"])
    same(free["mraw"], [[-20.0]])                        # e = (-32, -20): cell 1 limits
    r = cr.step(ucmd, soc, v, S, 10.0, NAN, balance=bal)
    same(r["istr"], [[-10.0]]); same(r["u"], [[-8.0, -10.0]])           # a_c = m' + b_c for the bleeding cell
    same(r["limiter"], np.array([[-2]], dtype=np.int32))
    same(r["st"]["pack"]["headroom"], [-10.0 - (-32.0), -10.0 - (-20.0)])
    same(r["st"]["pack"]["nlim"], [0.0, 0.0])
    for k in br.FIELDS:                                   # the balance record is the balancer's own
        same(r["st"]["bal"][k], b[k], k)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("balanced", [False, True])
def test_identities(S, balanced):
    rng = np.random.Generator(np.random.PCG64(5))
    N, n = 6, 8
    ucmd = -rng.uniform(1.0, 30.0, (N, n))
    ucmd[2, 3] = NAN
    ucmd[4, :4] = NAN
    soc = rng.uniform(0.2, 0.6, (N, n))
    v = rng.uniform(3.0, 4.0, (N, n))
    bal = (np.full(n, 1.5), np.full(n, 0.05), np.full(n, 0.02), 1) if balanced else None
    plain = br.step(ucmd, soc, S, *bal) if balanced else pr.reduce(ucmd, S)
    for par in ((NAN, NAN), (np.inf, np.inf), (NAN, np.inf)):
        r = cr.step(ucmd, soc, v, S, *par, balance=bal)
        same(r["u"], plain["u"]); same(r["limiter"], plain["limiter"])
        for k in pr.FIELDS:
            same(r["st"]["pack"][k], plain[k], k)
        if balanced:
            same(r["bleed"], plain["bleed"]); same(r["zmin"], plain["zmin"])
            for k in br.FIELDS:
                same(r["st"]["bal"][k], plain[k], k)
        assert (r["capby"] <= 0).all() and (r["st"]["charger"]["curtail"] == 0).all()
    if S == 1:                                            # V_g = v + 0.0
        r = cr.step(ucmd, soc, v, 1, NAN, NAN)
        same(r["vstr"], np.where(np.isnan(ucmd), 0.0, v + 0.0))
