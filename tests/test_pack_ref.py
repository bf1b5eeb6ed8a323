"""CPU: tests/pack_ref.py, the numpy restatement of include/mpcekf.h's series-string rule, on
hand-written cases: a tie, -0.0 against +0.0, a NaN cell in the middle of a string, an all-NaN
string, S = 1, the record across steps and across calls.  Every expected value below is written
out by hand from the header's rule."""
import numpy as np
import pytest

import pack_ref as pr

NaN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def test_largest_command_wins_and_is_copied_bit_for_bit():
    # charging current is negative: the largest command is the smallest charging current
    ucmd = np.array([[-3.0, -1.25, -2.0, -0.5, -4.0, -4.5]])
    r = pr.reduce(ucmd, 3)
    assert r["limiter"].dtype == np.int32 and r["limiter"].tolist() == [[1, 0]]
    assert same_bits(r["u"], [[-1.25, -1.25, -1.25, -0.5, -0.5, -0.5]])
    assert r["nlim"].tolist() == [0, 1, 0, 1, 0, 0]
    assert r["steps"].tolist() == [1, 1, 1, 1, 1, 1]
    assert r["headroom"].tolist() == [1.75, 0.0, 0.75, 0.0, 3.5, 4.0]    # m_g - u_c


def test_tie_goes_to_the_lowest_index():
    ucmd = np.array([[-2.0, -1.0, -1.0, -1.0], [-1.0, -1.0, -3.0, -1.0]])
    r = pr.reduce(ucmd, 4)
    assert r["limiter"].tolist() == [[1], [0]]
    assert r["nlim"].tolist() == [1, 1, 0, 0]
    assert same_bits(r["u"], np.full((2, 4), -1.0))
    assert r["headroom"].tolist() == [1.0, 0.0, 2.0, 0.0]


def test_negative_zero_equals_positive_zero_and_the_limiters_bits_are_kept():
    r = pr.reduce(np.array([[-1.0, -0.0, 0.0], [-1.0, 0.0, -0.0]]), 3)
    assert r["limiter"].tolist() == [[1], [1]]                           # equal by value: lowest index
    assert same_bits(r["u"][0], [-0.0, -0.0, -0.0]) and same_bits(r["u"][1], [0.0, 0.0, 0.0])
    assert not same_bits(r["u"][0], r["u"][1])
    assert r["nlim"].tolist() == [0, 2, 0]
    assert r["headroom"].tolist() == [2.0, 0.0, 0.0] and not np.signbit(r["headroom"]).any()


def test_nan_cell_in_the_middle_is_excluded_and_keeps_its_nan():
    ucmd = np.array([[-3.0, NaN, -2.0], [NaN, NaN, -5.0]])
    r = pr.reduce(ucmd, 3)
    assert r["limiter"].tolist() == [[2], [2]]
    assert same_bits(r["u"], [[-2.0, NaN, -2.0], [NaN, NaN, -5.0]])
    assert r["steps"].tolist() == [1, 0, 2]
    assert r["nlim"].tolist() == [0, 0, 2]
    assert r["headroom"].tolist() == [1.0, 0.0, 0.0]
    # a NaN in front of the winner does not win a tie either
    assert pr.reduce(np.array([[NaN, -1.0, -1.0]]), 3)["limiter"].tolist() == [[1]]


def test_all_nan_string_writes_nothing():
    ucmd = np.array([[NaN, NaN, -1.0, -2.0]])
    r = pr.reduce(ucmd, 2)
    assert r["limiter"].tolist() == [[-1, 0]]
    assert same_bits(r["u"], [[NaN, NaN, -1.0, -1.0]])
    assert r["steps"].tolist() == [0, 0, 1, 1] and r["nlim"].tolist() == [0, 0, 1, 0]
    assert r["headroom"].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_series_one_is_the_identity():
    ucmd = np.array([[-3.0, NaN, -0.0], [-2.5, NaN, 1.0]])
    r = pr.reduce(ucmd, 1)
    assert same_bits(r["u"], ucmd)
    assert r["limiter"].tolist() == [[0, -1, 0], [0, -1, 0]]
    assert np.array_equal(r["nlim"], r["steps"]) and r["steps"].tolist() == [2, 0, 2]
    assert r["headroom"].tolist() == [0.0, 0.0, 0.0]


def test_only_finite_terms_are_added():
    inf = float("inf")
    r = pr.reduce(np.array([[inf, -1.0], [-inf, -1.0], [-1.0, -3.0]]), 2)
    assert r["limiter"].tolist() == [[0], [1], [0]]
    # step 0: inf - inf is NaN and inf - (-1) is inf: neither added; step 1: -1 - (-inf) is inf
    assert r["headroom"].tolist() == [0.0, 2.0]
    assert r["steps"].tolist() == [3, 3] and r["nlim"].tolist() == [2, 1]


def test_headroom_is_the_sequential_sum_and_accumulates_across_calls():
    a, b, c = 0.1, 0.2, 0.3
    ucmd = np.array([[0.0, -a], [0.0, -b], [0.0, -c]])
    r = pr.reduce(ucmd, 2)
    assert r["headroom"][1] == ((0.0 + (0.0 - -a)) + (0.0 - -b)) + (0.0 - -c)
    assert r["headroom"][1] != (0.0 - -a) + ((0.0 - -b) + (0.0 - -c))      # the order reaches the bits
    r1 = pr.reduce(ucmd[:1], 2)
    r2 = pr.reduce(ucmd[1:], 2, state=r1)
    for k in pr.FIELDS:
        assert same_bits(r2[k], r[k]), k
    assert same_bits(np.concatenate([r1["u"], r2["u"]]), r["u"])


def test_bad_series_is_refused():
    for S in (0, -1, 4):
        with pytest.raises(ValueError, match="series"):
            pr.reduce(np.zeros((1, 6)), S)
