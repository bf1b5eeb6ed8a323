"""CPU: tests/term_ref.py, the termination rule of include/mpcekf.h in plain numpy, on hand-built
rows whose outcome can be read off the header's rule by eye."""
import numpy as np

import term_ref as tr

NaN = float("nan")


def run(rows, series=None, **kw):
    """rows: a list of (z, u, T) per step, each [n].  Returns (the u rows after the rule, state)."""
    n = len(rows[0][0])
    st, out = tr.reset(n), []
    for z, u, T in rows:
        o, st = tr.step(st, z, u, T, series=series, **kw)
        out.append(o)
    return np.stack(out), st


def test_each_reason_bit_alone_and_combined():
    # cells: 0 none, 1 soc, 2 taper, 3 temp, 4 soc + temp, 5 all three
    z = np.array([0.5, 0.9, 0.5, 0.5, 0.9, 0.9])
    T = np.array([25.0, 25.0, 25.0, 45.0, 45.0, 45.0])
    u1 = np.full(6, -6.0)                                  # arms every taper counter
    u2 = np.array([-6.0, -6.0, -0.5, -6.0, -6.0, -0.5])
    calm = (np.full(6, 0.5), u1, np.full(6, 25.0))
    out, st = run([calm, (z, u2, T)], soc_stop=0.8, i_taper=1.0, hold=1, T_cut=40.0)
    assert st["reason"].tolist() == [0, 1, 2, 4, 5, 7]
    assert st["state"].tolist() == [0, 1, 1, 1, 1, 1]
    assert st["done_step"].tolist() == [0, 2, 2, 2, 2, 2]
    assert st["steps"].tolist() == [2] * 6 and st["rest"].tolist() == [0, 1, 1, 1, 1, 1]
    assert np.array_equal(st["soc_done"][1:], z[1:]) and np.isnan(st["soc_done"][0])
    assert np.array_equal(st["u_done"][1:], u2[1:]) and np.array_equal(st["T_done"][1:], T[1:])
    assert np.array_equal(out[0], u1) and out[1].tolist() == [-6.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert tr.n_open(st) == 1
    # thresholds are inclusive: z == soc_stop and T == T_cut latch
    _, st = run([(np.array([0.8, 0.5]), np.array([-6.0, -6.0]), np.array([25.0, 40.0]))], soc_stop=0.8, T_cut=40.0)
    assert st["reason"].tolist() == [1, 4]


def test_nan_thresholds_turn_a_criterion_off():
    rows = [(np.full(3, 0.99), np.full(3, -6.0), np.full(3, 90.0)), (np.full(3, 0.99), np.full(3, 0.0), np.full(3, 90.0))]
    _, st = run(rows)                                                       # all off
    assert (st["state"] == tr.OPEN).all() and (st["steps"] == 2).all() and (st["rest"] == 0).all()
    _, st = run(rows, soc_stop=np.array([NaN, 0.5, NaN]), i_taper=NaN, T_cut=np.array([NaN, NaN, 50.0]))
    assert st["state"].tolist() == [0, 1, 1] and st["reason"].tolist() == [0, 1, 4] and st["done_step"].tolist() == [0, 1, 1]


def test_taper_counter():
    def taper(us, hold):
        rows = [(np.array([0.5]), np.array([u]), np.array([25.0])) for u in us]
        out, st = run(rows, i_taper=1.0, hold=hold)
        return out[:, 0].tolist(), int(st["done_step"][0]), int(st["reason"][0])
    # un-armed at the start: small currents from the first step on never count
    assert taper([-0.5, -0.5, 0.0, -0.9], 1) == ([-0.5, -0.5, 0.0, -0.9], 0, 0)
    # hold = 1: the first step at or under the threshold after one above it (|u| == i_taper counts)
    assert taper([-0.5, -3.0, -1.0, -0.2], 1) == ([-0.5, -3.0, 0.0, 0.0], 3, 2)
    # hold = 3: three in a row
    assert taper([-3.0, -0.9, -0.8, -0.7, -0.6], 3) == ([-3.0, -0.9, -0.8, 0.0, 0.0], 4, 2)
    # a run broken by one large |u| starts again (discharge counts by magnitude)
    assert taper([-3.0, -0.9, -0.8, 2.0, -0.7, -0.6, -0.5, -0.4], 3) == ([-3.0, -0.9, -0.8, 2.0, -0.7, -0.6, 0.0, 0.0], 7, 2)


def test_dead_cells():
    z = np.array([NaN, 0.9, 0.9, 0.5])
    u = np.array([-6.0, NaN, -6.0, -6.0])
    out, st = run([(z, u, np.full(4, 25.0))] * 2, soc_stop=0.8)
    assert st["state"].tolist() == [2, 2, 1, 0] and st["done_step"].tolist() == [1, 1, 1, 0]
    assert st["reason"].tolist() == [0, 0, 1, 0] and st["steps"].tolist() == [1, 1, 1, 2]
    assert np.isnan(st["soc_done"][:2]).all() and st["rest"].tolist() == [0, 0, 2, 0]
    assert out[1, 0] == -6.0 and np.isnan(out[1, 1])       # a dead cell's command is never touched
    assert tr.n_open(st) == 1


def test_dead_wins_over_the_string_flag():
    # one string of 3: cell 0 latches at step 1; at step 2 cell 1 has a NaN command, cell 2 follows
    z1, z2 = np.array([0.9, 0.5, 0.5]), np.array([0.9, 0.5, 0.5])
    u1, u2 = np.full(3, -6.0), np.array([-6.0, NaN, -6.0])
    out, st = run([(z1, u1, np.full(3, 25.0)), (z2, u2, np.full(3, 25.0))], series=3, soc_stop=0.8)
    assert st["state"].tolist() == [1, 2, 1] and st["reason"].tolist() == [1, 0, 8]
    assert st["done_step"].tolist() == [1, 2, 2]


def test_string_lag_is_exactly_one_step():
    # two strings of 2; cell 0 latches at step 2; its mate at step 3, not 2; the other string never
    T = np.full(4, 25.0)
    u = np.full(4, -6.0)
    rows = [(np.array([0.5, 0.5, 0.5, 0.5]), u, T), (np.array([0.9, 0.5, 0.5, 0.5]), u, T),
            (np.array([0.9, 0.5, 0.5, 0.5]), u, T), (np.array([0.9, 0.5, 0.5, 0.5]), u, T)]
    out, st = run(rows, series=2, soc_stop=0.8)
    assert st["done_step"].tolist() == [2, 3, 0, 0] and st["reason"].tolist() == [1, 8, 0, 0]
    assert out[:, 1].tolist() == [-6.0, -6.0, 0.0, 0.0]    # the mate's own command stands during the lag step
    assert st["rest"].tolist() == [3, 2, 0, 0] and st["steps"].tolist() == [2, 3, 4, 4]
    assert st["soc_done"][1] == 0.5 and st["u_done"][1] == -6.0
    # without a pack, and at series = 1, nobody follows
    for S in (None, 1):
        _, st = run(rows, series=S, soc_stop=0.8)
        assert st["done_step"].tolist() == [2, 0, 0, 0]


def test_latched_nan_command_is_left_alone_and_minus_zero_is_overwritten():
    T = np.full(2, 25.0)
    rows = [(np.array([0.9, 0.9]), np.array([-0.0, -6.0]), T), (np.array([0.9, 0.9]), np.array([-0.0, NaN]), T),
            (np.array([NaN, 0.9]), np.array([-0.0, -0.0]), T)]
    out, st = run(rows, soc_stop=0.8)
    assert st["done_step"].tolist() == [1, 1] and st["state"].tolist() == [1, 1]   # latched stays latched, NaN or not
    assert not np.signbit(out[:, 0]).any() and (out[:, 0] == 0).all()              # -0.0 -> +0.0
    assert np.signbit(st["u_done"][0]) and st["u_done"][0] == 0                    # the record keeps the command's bits
    assert np.isnan(out[1, 1]) and out[2, 1] == 0 and not np.signbit(out[2, 1])
    assert st["rest"].tolist() == [3, 2]


def test_step_does_not_modify_its_state_argument():
    st = tr.reset(2)
    _, st2 = tr.step(st, np.array([0.9, 0.5]), np.array([-6.0, -6.0]), np.array([25.0, 25.0]), soc_stop=0.8)
    assert st["t"] == 0 and (st["state"] == 0).all() and st2["t"] == 1 and st2["state"].tolist() == [1, 0]
    assert tuple(tr.record(st2)) == tr.FIELDS
