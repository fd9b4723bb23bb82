"""tests/noise_draw_cases.py, the numpy restatement of the device's noise draw (ddp-generator_amd/csrc/k_noise.inc), pinned
without a GPU: Philox4x32-10 to Random123's three known answers; the normals of one table to N(0, 1) in mean, variance,
correlation between components and lag-1 correlation along every axis of the counter; and every deliberate mistake of
noise_draw_cases.MUTANTS shown to miss the bar tests/test_gpu_policy_drawn.py holds the device to, 1e-12 sigma per entry, by a
factor of 1e6 or more — so that test can tell each of them from the recipe.

The moment bars are 5 standard deviations of each statistic under N(0, 1) for n = 262 144 independent normals: the mean has
standard deviation 1 / sqrt(n), the variance sqrt(2 / n), a correlation of two components over n / 4 pairs 1 / sqrt(n / 4), a
lag-1 mean product over about n pairs 1 / sqrt(n).  They are conditions, not measurements.  Measured here: 0.09, 0.37, 1.72 and, along k / r / b,
1.77 / 1.08 / 0.68.  (The issue that asked for the draw quotes 0.68 / 1.05 / 1.75 along k / r / b for its own restatement: the
reverse order.  With B = N = 64 a restatement that has k and the trajectory in each other's counter words produces the transposed
table, so the same three numbers in the other order; the small differences are the estimator's.  This file follows the
written definition, counter = (k, r, t, j), which Random123's known answers cannot decide and the device shares.)"""
import numpy as np
import pytest

from noise_draw_cases import MUTANTS, normals, philox4x32_10, table

SEED = 20261021
B, R, N, NX = 64, 16, 64, 4
BAR = 1e-12  # tests/test_gpu_policy_drawn.py: |d| <= BAR * sigma[i] per entry


def words(text):
    return np.array([int(w, 16) for w in text.split()], dtype=np.uint64)


@pytest.mark.parametrize("counter,key,output", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_gives_random123s_known_answers(counter, key, output):
    got = philox4x32_10(words(counter), words(key))
    assert got.dtype == np.uint32 and got.tolist() == words(output).tolist(), [hex(int(w)) for w in got]


def test_philox_is_elementwise():
    """a stack of counters under a stack of keys gives the stack of the single results"""
    c = np.stack([words("00000000 00000000 00000000 00000000"), words("243f6a88 85a308d3 13198a2e 03707344")])
    k = np.stack([words("00000000 00000000"), words("a4093822 299f31d0")])
    assert philox4x32_10(c, k).tolist() == [philox4x32_10(c[0], k[0]).tolist(), philox4x32_10(c[1], k[1]).tolist()]


def test_normals_of_the_extreme_words():
    """the smallest word gives the longest tail, 6.76 sigma, and nothing is ever infinite; the largest gives rho = 1.5e-5"""
    z = normals(np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32))[0]
    rho = np.sqrt(-2.0 * np.log(2.0 ** -33))
    assert np.all(np.isfinite(z)) and 6.7 < rho < 6.77
    assert abs(np.hypot(z[0], z[1]) - rho) < 1e-14 and abs(np.hypot(z[2], z[3]) - np.sqrt(-2.0 * np.log1p(-2.0 ** -33))) < 1e-14


@pytest.fixture(scope="module")
def unit():
    w = table(B, R, N, NX, SEED, np.ones(NX))
    assert w.shape == (B, R, N, NX) and w.size == 262144 and np.all(np.isfinite(w))
    return w


def test_mean_and_variance(unit):
    n = unit.size
    mean, var = abs(unit.mean()) * np.sqrt(n), abs(unit.var() - 1.0) / np.sqrt(2.0 / n)
    print("|mean| sqrt(n) = %.3g, |var - 1| / sqrt(2 / n) = %.3g" % (mean, var))
    assert mean <= 5.0 and var <= 5.0


def test_components_are_uncorrelated(unit):
    n = unit.size
    c = np.corrcoef(unit.reshape(-1, NX).T)
    worst = float(np.max(np.abs(c - np.eye(NX)))) * np.sqrt(n / 4)
    print("worst cross-component correlation times sqrt(n / 4) = %.3g" % worst)
    assert worst <= 5.0


@pytest.mark.parametrize("axis,name", [(2, "k"), (1, "r"), (0, "b")])
def test_neighbours_along_the_counter_are_uncorrelated(unit, axis, name):
    x = np.moveaxis(unit, axis, 0)
    lag = abs(float(np.mean(x[:-1] * x[1:]))) * np.sqrt(unit.size)
    print("lag-1 correlation along %s times sqrt(n) = %.3g" % (name, lag))
    assert lag <= 5.0


def test_table_layout_scaling_and_sharing():
    sigma = np.array([0.5, 2.0, 0.0, 1e-3, 3.0, 0.25, 1.0])
    w = table(3, 2, 5, 7, SEED, sigma, first=11)  # nx = 7: a whole block and a partial one
    assert w.shape == (3, 2, 5, 7) and np.all(w[..., 2] == 0.0)
    assert np.array_equal(w, sigma * table(3, 2, 5, 7, SEED, np.ones(7), first=11))
    assert np.array_equal(w[..., :4], table(3, 2, 5, 4, SEED, sigma[:4], first=11))       # (components >= nx are dropped)
    assert np.array_equal(w[1:], table(2, 2, 5, 7, SEED, sigma, first=12))                 # (the trajectory word is global)
    assert np.array_equal(w[:, :1], table(3, 1, 5, 7, SEED, sigma, first=11))              # (bits do not depend on R)
    shared = table(3, 2, 5, 7, SEED, sigma, shared=True, first=11)
    assert shared.shape == (2, 5, 7) and np.array_equal(shared, table(1, 2, 5, 7, SEED, sigma, first=0)[0])
    assert not np.array_equal(w, table(3, 2, 5, 7, SEED + (1 << 32), sigma, first=11))     # (both halves of the seed are key)
    assert not np.array_equal(w, table(3, 2, 5, 7, SEED + 1, sigma, first=11))
    top = table(2, 1, 2, 4, SEED, np.ones(4), first=2 ** 32 - 2)                          # (the last trajectory word)
    assert np.all(np.isfinite(top)) and not np.array_equal(top[0], top[1])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_misses_the_device_bar_a_million_times(mutant):
    sigma = np.array([0.5, 2.0, 0.0, 1e-3])
    ref = table(B, R, N, NX, SEED, sigma, first=7)
    got = table(B, R, N, NX, SEED, sigma, first=7, mutant=mutant)
    live = sigma > 0
    miss = float(np.max(np.abs(got - ref)[..., live] / sigma[live]))
    print("%s: worst |d| / sigma = %.3g, %.3g times the bar" % (mutant, miss, miss / BAR))
    assert miss >= 1e6 * BAR
