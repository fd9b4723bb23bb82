"""The numpy statement of tests/bestof_cases.py, checked directly: it is what tests/test_gpu_best_of.py holds k_best_of and
k_shift_winners_* to, so its own rules are pinned here on hand-written cases."""
import numpy as np
import pytest

from bestof_cases import DERIVS_FAILED, INIT_FAILED, best_of_rule, shift_winners_rule


def test_ties_resolve_to_the_lowest_index():
    w, best, n = best_of_rule([3.0, 1.0, 1.0, 2.0, 5.0, 5.0, 5.0, 5.0], np.zeros(8, dtype=int), 4)
    assert list(w) == [1, 4] and list(best) == [1.0, 5.0] and list(n) == [4, 4]
    w, _, _ = best_of_rule([2.0, 2.0, 1.0, 1.0], np.zeros(4, dtype=int), 2)
    assert list(w) == [0, 2]


def test_negative_zero_ties_with_zero():
    w, best, _ = best_of_rule([0.0, -0.0, -0.0, 0.0], np.zeros(4, dtype=int), 2)
    assert list(w) == [0, 2]
    assert not np.signbit(best[0]) and np.signbit(best[1])  # best is the winner's own score


def test_nan_and_both_infinities_are_ineligible():
    w, best, n = best_of_rule([np.nan, np.inf, -np.inf, 7.0], np.zeros(4, dtype=int), 4)
    assert list(w) == [3] and list(best) == [7.0] and list(n) == [1]


def test_status_7_is_ineligible_and_status_6_is_not():
    w, best, n = best_of_rule([1.0, 2.0, 1.0, 2.0], [INIT_FAILED, 0, DERIVS_FAILED, 0], 2)
    assert list(w) == [1, 2] and list(best) == [2.0, 1.0] and list(n) == [1, 2]


def test_a_segment_without_an_eligible_slot():
    w, best, n = best_of_rule([np.nan, 1.0, 3.0, 2.0], [0, INIT_FAILED, 0, 0], 2)
    assert list(w) == [-1, 3] and np.isnan(best[0]) and best[1] == 2.0 and list(n) == [0, 2]


def test_k_1_every_slot_is_its_segment():
    w, best, n = best_of_rule([4.0, np.inf, 2.0], [0, 0, INIT_FAILED], 1)
    assert list(w) == [0, -1, -1] and best[0] == 4.0 and np.all(np.isnan(best[1:])) and list(n) == [1, 0, 0]


def test_sizes_are_checked():
    for score, K in (([1.0, 2.0, 3.0], 2), ([1.0, 2.0, 3.0], 3)):
        with pytest.raises(AssertionError):
            best_of_rule(score, np.zeros(3, dtype=int), K)


def test_the_composed_shift():
    B, N, nx, nu, K = 4, 5, 3, 2, 2
    rng = np.random.default_rng(2)
    x, u = rng.standard_normal((B, N + 1, nx)), rng.standard_normal((B, N, nu))
    x0, un = shift_winners_rule(x, u, K, [1, -1], 2)
    # segment 0 takes slot 1's plan, the last control held; segment 1's slots keep their own
    for b, w in ((0, 1), (1, 1), (2, 2), (3, 3)):
        assert np.array_equal(un[b, :3], u[w, 2:]) and np.array_equal(un[b, 3], u[w, 4]) and np.array_equal(un[b, 4], u[w, 4])
        assert np.array_equal(x0[b], x[w, 2])
    x0_new, tail, du = rng.standard_normal((2, nx)), rng.standard_normal((2, 2, nu)), rng.standard_normal((B, N, nu))
    du[1] = 0.0  # the incumbent stays as it is
    x0, un = shift_winners_rule(x, u, K, [1, 2], 2, x0_new, tail, du)
    for b, w in ((0, 1), (1, 1), (2, 2), (3, 2)):
        g = b // K
        assert np.array_equal(un[b], np.concatenate([u[w, 2:], tail[g]]) + du[b]) and np.array_equal(x0[b], x0_new[g])
    assert np.array_equal(un[1], np.concatenate([u[1, 2:], tail[0]]))
    # steps = 0, own plans, nothing added: the identity, bit for bit (-0.0 included)
    u[0, 0, 0] = -0.0
    x0, un = shift_winners_rule(x, u, K, [-1, -1], 0)
    assert np.array_equal(x0, x[:, 0]) and np.array_equal(un, u) and np.signbit(un[0, 0, 0])
    with pytest.raises(AssertionError):
        shift_winners_rule(x, u, K, [2, -1], 1)  # a winner outside its segment
