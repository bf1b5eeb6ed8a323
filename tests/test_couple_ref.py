"""CPU: tests/couple_ref.py, the numpy restatement of include/mpcekf.h's heat conduction between
neighbouring cells of a pack string, against cases worked out by hand from the header's rule.

The cases keep every cell's own heat at zero (i = 0, so q = 0 * (U - v) = 0; Rth = +inf, so
loss = 0) with Ts = 1 s and Cth = 2 J/K: Tn = T + qn / 2, and every expected value below is a
short binary fraction written out from the rule, none computed by the code under test.
"""
import numpy as np

import couple_ref as cr

OCV = np.array([3.0, 4.0])


def run(T0, r_link, S, nsteps, rec=None, error=None, i=0.0, Rth=np.inf, Tamb=0.0):
    n = len(T0)
    p = dict(Cth=np.full(n, 2.0), Rth=np.full(n, Rth), Tamb=np.full(n, Tamb))
    u = np.full((nsteps, n), i)
    return cr.restate(1.0, 0.0, 1.0, p, OCV, np.asarray(r_link, dtype=np.float64), S, np.asarray(T0, dtype=np.float64),
                      np.full(n, i), u, np.ones((nsteps, n)), np.full((nsteps, n), 0.5), np.full(n, 0.5), rec=rec,
                      error=error)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def exact(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), (what, got, want)


def test_two_cell_string():
    temp, heat, cond, th, cp = run([20.0, 24.0], [2.0, 7.0], 2, 2)   # the string's last entry (7) is ignored
    exact(cond, [[2.0, -2.0], [1.0, -1.0]], "cond")                   # (24-20)/2, then (23-21)/2
    exact(temp, [[20.0, 24.0], [21.0, 23.0]], "temp")
    exact(th["T"], [21.5, 22.5], "T")
    exact(heat, np.zeros((2, 2)), "heat")
    exact(cp["NB_SUM"], [3.0, -3.0], "NB_SUM")
    exact(cp["DT_MAX"], [4.0, 4.0], "DT_MAX")
    exact(cp["DT_MAX_STEP"], [1.0, 1.0], "DT_MAX_STEP")
    exact(th["steps"], [2.0, 2.0], "steps")


def test_three_cell_string_end_cells_have_one_link():
    temp, heat, cond, th, cp = run([20.0, 24.0, 30.0], [2.0, 4.0, 1.0], 3, 1)
    # cell 1: dl = -4, -4/2 = -2; dr = 6, 6/4 = 1.5; qn = (0 + -2) + 1.5
    exact(cond, [[2.0, -0.5, -1.5]], "cond")
    exact(th["T"], [21.0, 23.75, 29.25], "T")
    exact(cp["DT_MAX"], [4.0, 6.0, 6.0], "DT_MAX")           # the middle cell: |dl| = 4, then |dr| = 6 > 4
    qn, nl, *_ = cr.conduct(np.array([20.0, 24.0, 30.0]), np.array([2.0, 4.0, 1.0]), 3)
    assert nl.tolist() == [1, 2, 1]
    # two strings side by side do not conduct across the string boundary
    _, _, cond2, th2, _ = run([20.0, 24.0, 30.0, 50.0, 50.0, 50.0], [2.0, 4.0, 1.0, 1.0, 1.0, 1.0], 3, 1)
    exact(cond2, [[2.0, -0.5, -1.5, 0.0, 0.0, 0.0]], "two strings")
    exact(th2["T"], [21.0, 23.75, 29.25, 50.0, 50.0, 50.0], "two strings: T")


def test_inf_link_in_the_middle():
    T0, r = [20.0, 24.0, 30.0, 34.0], [2.0, np.inf, 2.0, 1.0]
    _, _, cond, th, cp = run(T0, r, 4, 1)
    exact(cond, [[2.0, -2.0, 2.0, -2.0]], "cond")
    exact(th["T"], [21.0, 23.0, 31.0, 33.0], "T")
    exact(cp["DT_MAX"], [4.0, 4.0, 4.0, 4.0], "DT_MAX")       # 30 - 24 = 6 over the missing link is not seen
    _, nl, dl, dr, _, _ = cr.conduct(np.array(T0), np.array(r), 4)
    assert nl.tolist() == [1, 1, 1, 1] and np.isnan(dr[1]) and np.isnan(dl[2])


def test_no_link_gives_the_uncoupled_bits():
    """q - loss = -0.0 and T = -0.0: the uncoupled line gives -0.0, the coupled one with qn = +0.0
    would give +0.0.  A cell with nl == 0 must take the first."""
    for r, S in (([np.inf, np.inf], 2), ([1.0, 1.0], 1)):
        _, heat, cond, th, cp = run([-0.0, -0.0], r, S, 1, i=-0.0, Rth=2.0, Tamb=-0.0)
        assert np.signbit(heat).all() and (heat == 0).all()           # q = -0.0 * (3.5 - 1)
        exact(th["T"], [-0.0, -0.0], "T")
        exact(cond, [[0.0, 0.0]], "cond is +0.0")
        exact(cp["NB_SUM"], [0.0, 0.0], "NB_SUM")
        exact(cp["DT_MAX"], [np.nan, np.nan], "DT_MAX")
        exact(cp["DT_MAX_STEP"], [0.0, 0.0], "DT_MAX_STEP")
    p = dict(Cth=np.full(2, 2.0), Rth=np.full(2, 2.0), Tamb=np.full(2, -0.0))
    T = np.array([-0.0, -0.0])
    a = cr.model_step(T, np.full(2, -0.0), np.ones(2), np.full(2, 0.5), p, OCV, 0.0, 1.0, 1.0)
    b = cr.model_step(T, np.full(2, -0.0), np.ones(2), np.full(2, 0.5), p, OCV, 0.0, 1.0, 1.0, np.zeros(2),
                      np.zeros(2, dtype=np.int64))
    c = cr.model_step(T, np.full(2, -0.0), np.ones(2), np.full(2, 0.5), p, OCV, 0.0, 1.0, 1.0, np.zeros(2),
                      np.ones(2, dtype=np.int64))
    exact(a[2], b[2], "nl == 0 is the uncoupled line")
    assert np.signbit(a[2]).all() and not np.signbit(c[2]).any()


def test_exact_cancellation_over_a_link():
    rng = np.random.Generator(np.random.PCG64(0xC0))
    n = 64
    T0, r = rng.uniform(-20.0, 60.0, n), rng.uniform(0.5, 5.0, n)
    _, _, cond, _, cp = run(T0, r, 2, 5)
    assert (bits(cond[:, 0::2]) == bits(-cond[:, 1::2])).all() and (cond[0] != 0).all()
    exact(cp["NB_SUM"][0::2], -cp["NB_SUM"][1::2], "NB_SUM")


def test_held_cell_still_conducts():
    temp, heat, cond, th, cp = run([20.0, 24.0], [2.0, 1.0], 2, 2, error=np.array([True, False]))
    assert np.isnan(heat[:, 0]).all() and (heat[:, 1] == 0).all()
    exact(temp, [[20.0, 24.0], [20.0, 23.0]], "temp")                 # cell 0 held, cell 1 cooled by it
    exact(cond, [[2.0, -2.0], [1.5, -1.5]], "cond")
    exact(th["T"], [20.0, 22.25], "T")
    exact(th["nheld"], [2.0, 0.0], "nheld")
    exact(cp["NB_SUM"], [3.5, -3.5], "NB_SUM")


def test_record_across_steps_and_calls():
    _, _, _, th, cp = run([20.0, 24.0], [2.0, 1.0], 2, 2)
    # a second call continues: step 3 from T = [21.5, 22.5]
    _, _, cond, th, cp = run(th["T"], [2.0, 1.0], 2, 1, rec=(th, cp))
    exact(cond, [[0.5, -0.5]], "cond")
    exact(cp["NB_SUM"], [3.5, -3.5], "NB_SUM")
    exact(cp["DT_MAX"], [4.0, 4.0], "DT_MAX")
    exact(cp["DT_MAX_STEP"], [1.0, 1.0], "DT_MAX_STEP")
    exact(th["steps"], [3.0, 3.0], "steps")
    # an equal gradient later does not replace (strict >); a larger one does, with the model's step index
    _, _, _, th, cp = run([20.0, 24.0], [2.0, 1.0], 2, 1, rec=(th, cp))
    exact(cp["DT_MAX_STEP"], [1.0, 1.0], "DT_MAX_STEP after an equal gradient")
    _, _, _, th, cp = run([10.0, 30.0], [2.0, 1.0], 2, 1, rec=(th, cp))
    exact(cp["DT_MAX"], [20.0, 20.0], "DT_MAX")
    exact(cp["DT_MAX_STEP"], [5.0, 5.0], "DT_MAX_STEP")
    exact(cp["NB_SUM"], [15.5, -15.5], "NB_SUM")                      # 3.5 + 2 + 10
