"""tests/isotonic_exact.py against itself and against sklearn: the hull form equals textbook pool-adjacent-violators block for
block, both are the isotonic regression sklearn computes, and the fit has the properties that make it a recalibration map."""
import fractions

import numpy as np
import pytest

from isotonic_exact import block_values, isotonic_apply, isotonic_exact, isotonic_rows, isotonic_rows_slow


def patterns(n):
    """(name, labels) on n increasing scores: the shapes the device tests use"""
    rng = np.random.default_rng(n)
    stair = np.concatenate([np.r_[1, np.zeros(m - 1, np.int64)] for m in range(int((2 * n) ** 0.5) + 2, 0, -1)])[:n]
    late = (rng.random(n) < 0.5).astype(np.int64)
    late[n - n // 8:] = 0
    return [("one-block", (np.arange(n) < n // 2).astype(np.int64)), ("staircase", stair), ("sawtooth", (np.arange(n) % 2 == 0).astype(np.int64)),
            ("late pull-back", late)]


def _cases():
    rng = np.random.default_rng(0)
    out = []
    for trial in range(120):
        n = int(rng.integers(1, 300))
        if trial % 3 == 0:
            p = rng.random(n).astype(np.float32)
        elif trial % 3 == 1:
            p = rng.choice(np.linspace(-0.5, 1.5, int(rng.integers(1, 40))).astype(np.float32), n)      # tie runs, scores outside [0, 1]
        else:
            p = rng.choice(np.array([-0.0, 0.0, 0.25, 0.5], np.float32), n)
        out.append(((rng.random(n) < 0.1 + 0.6 * np.clip(p, 0, 1)).astype(np.int64), p))
    for n in (1, 2, 3, 63, 64, 65, 257):
        out += [(y, np.arange(n, dtype=np.float32)) for _, y in patterns(n) if len(y) == n]
    return out


def _same(a, b):
    return [(float(x[0]), float(x[1]), int(x[2]), int(x[3])) for x in a] == [(float(x[0]), float(x[1]), int(x[2]), int(x[3])) for x in b]


def test_the_hull_form_is_pool_adjacent_violators():
    for y, p in _cases():
        assert _same(isotonic_rows(y, p), isotonic_rows_slow(y, p)), (y, p)


def test_hand_cases():
    assert _same(isotonic_rows([1], [0.3]), [(np.float32(0.3), np.float32(0.3), 1, 1)])
    assert _same(isotonic_rows([1, 0], [0.5, 0.5]), [(0.5, 0.5, 2, 1)])
    assert _same(isotonic_rows([1, 0, 1, 0], [1, 2, 3, 4]), [(1, 4, 4, 2)])                     # equal means are ONE block
    assert _same(isotonic_rows([0, 1, 0, 1], [1, 2, 3, 4]), [(1, 1, 1, 0), (2, 3, 2, 1), (4, 4, 1, 1)])
    b = isotonic_rows([1, 0], [-0.0, 0.0])
    assert _same(b, [(0.0, 0.0, 2, 1)]) and not np.signbit(b[0][0])
    # the documented five rows
    b = isotonic_rows([0, 1, 0, 1, 1], [0.125, 0.25, 0.25, 0.75, 1.0])
    assert _same(b, [(0.125, 0.125, 1, 0), (0.25, 0.25, 2, 1), (0.75, 1.0, 2, 2)])
    got = isotonic_apply(b, np.array([0.0, 0.125, 0.1875, 0.25, 0.5, 0.75, 2.0], np.float32))
    assert got.tolist() == [0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.0]
    assert isotonic_apply(b, np.array([0.0, 2.0], np.float32), eps=0.25).tolist() == [0.25, 0.75]


def test_properties():
    for y, p in _cases():
        b = isotonic_rows(y, p)
        v = [fractions.Fraction(x[3], x[2]) for x in b]
        assert all(v[i] < v[i + 1] for i in range(len(v) - 1))
        assert all(x[0] <= x[1] for x in b) and all(b[i][1] < b[i + 1][0] for i in range(len(b) - 1))
        assert sum(x[2] for x in b) == len(y)
        assert sum(vi * x[2] for vi, x in zip(v, b)) == int(np.sum(y))
        if float(np.min(p)) >= 0 and float(np.max(p)) <= 1:
            # Brier on the fit rows, exact: a block of c rows and s positives at value s / c costs s (1 - s/c)^2 + (c - s) (s/c)^2
            fit = sum(x[3] * (1 - vi) ** 2 + (x[2] - x[3]) * vi ** 2 for vi, x in zip(v, b))
            raw = sum((fractions.Fraction(float(pi)) - int(yi)) ** 2 for pi, yi in zip(p, y))
            assert fit <= raw


def test_segments():
    rng = np.random.default_rng(3)
    n = 500
    p = rng.random(n).astype(np.float32)
    y = (rng.random(n) < p).astype(np.int64)
    d = rng.choice([0, 2], n)
    fits = isotonic_exact(y, p, d, 3)
    assert len(fits) == 4 and fits[1] == [] and _same(fits[3], isotonic_rows(y, p)) and _same(fits[2], isotonic_rows(y[d == 2], p[d == 2]))


def test_against_sklearn():
    iso = pytest.importorskip("sklearn.isotonic")
    rng = np.random.default_rng(1)
    for y, p in _cases():
        b = isotonic_rows(y, p)
        ir = iso.IsotonicRegression(out_of_bounds="clip").fit(p.astype(np.float64), y.astype(np.float64))
        grid = np.r_[p, rng.uniform(float(p.min()) - 1, float(p.max()) + 1, 50).astype(np.float32)]
        # the exact map in float64 (no rounding to float32): the contract's operations
        lo = np.array([x[0] for x in b], np.float64)
        hi = np.array([x[1] for x in b], np.float64)
        xk = np.empty(2 * len(b))
        xk[0::2], xk[1::2] = lo, hi
        vk = np.repeat(block_values(b), 2)
        keep = np.r_[True, xk[1:] != xk[:-1]]
        want = np.interp(grid.astype(np.float64), xk[keep], vk[keep])
        assert np.abs(ir.predict(grid.astype(np.float64)) - want).max() <= 1e-12
        assert np.abs(isotonic_apply(b, grid).astype(np.float64) - want).max() <= 2.0 ** -24      # one rounding to float32 of a value in [0, 1]
