"""The f-statistics without a GPU: fmh_fstat_moment_count, fmh_fstat_f4 and fmh_block_jackknife against tests/fstat_ref.py (exact
fractions), and the Python surface that needs no device (FStatistics.from_moments / concatenate / f2_blocks, argument errors).

Tolerances.  With u = 2^-53:
  * fmh_fstat_f4 evaluates the biased part as one exact integer numerator and one exact integer denominator, each converted to f64 (one
    rounding each) and divided (one more), and every h term the same way with an exact denominator (two roundings); each h term is then
    added to the running sum (one rounding of a value no larger than |biased| + sum |h|).  That is at most four roundings per term; the
    bound asserted is twice that:  |got - exact| <= 2^-50 (|biased| + sum |h terms used|).
  * fmh_block_jackknife cancels (theta_J = g theta - sum ..., tau_j - theta_J), so its error is not a fixed count of roundings.  The largest
    relative deviation from the exact fractions over this file's fixed seeds was measured here on the CPU (JACKKNIFE_MEASURED below, per
    field) and the test asserts 16 times it - the margin covers compiler contraction differences between builds.
"""

import ctypes as C
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import fstat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# largest relative deviation of fmh_block_jackknife from the exact fractions over jackknife_cases(), measured on the CPU build
JACKKNIFE_MEASURED = {"estimate": 3.926e-16, "jackknife_estimate": 1.316e-13, "se": 2.767e-14, "z": 2.785e-14}
JACKKNIFE_MARGIN = 16


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import _abi

    return _abi.load()


@pytest.fixture(scope="module")
def dev(lib):
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm(lib):
    import ferromic

    return ferromic


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


# ---- symbols, options, the slice width ------------------------------------------------------------------------------------------------
def test_symbols_options_and_moment_count(lib, dev):
    from ferromic_amd import _abi

    for name, n_args in (("fmh_fstat_moments", 8), ("fmh_fstat_moment_count", 1), ("fmh_fstat_f4", 9), ("fmh_block_jackknife", 5)):
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_abi.JackknifeOut) == 5 * 8
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    assert "#define FMH_ABI_VERSION 3" in header and "#define FMH_FSTAT_MAX_GROUPS 32" in header and "fmh_jackknife_out" in header
    for key in ("FMH_FSTAT_ITEM_ROWS", "FMH_FSTAT_LDS_MASK_BYTES"):
        assert _abi.get_option(key) == 0 and key in header
        _abi.set_option(key, 7)
        assert _abi.get_option(key) == 7
        _abi.set_option(key, None)
        assert _abi.get_option(key) == 0
    for G in range(2, 33):
        assert dev.fstat_moment_count(G) == fstat_ref.moment_count(G) == 1 + G + G * (G + 1) // 2
    assert dev.fstat_moment_count(32) == 561
    for G in (-1, 0, 1, 33, 1 << 20):
        assert dev.fstat_moment_count(G) == 0
    # the slot order: the upper triangle row-major, diagonal included
    assert [fstat_ref.pair_slot(3, i, j) for i in range(3) for j in range(i, 3)] == [4, 5, 6, 7, 8, 9]
    assert fstat_ref.pair_slot(3, 2, 0) == fstat_ref.pair_slot(3, 0, 2) == 6


# ---- fmh_fstat_f4 ---------------------------------------------------------------------------------------------------------------------------
def cohort_table(rows, cols, sizes, seed):
    """A random complete cohort and groups of the given sizes (overlapping, drawn independently): (slice of all rows, sizes)."""
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, cols)) < rng.beta(0.5, 1.2, size=rows)[:, None]).astype(np.uint8)
    masks = np.zeros((len(sizes), cols), dtype=bool)
    for g, n in enumerate(sizes):
        masks[g, rng.choice(cols, size=n, replace=False)] = True
    table, multi, incomplete = fstat_ref.moments(x, None, masks, [(0, rows)])
    assert multi[0] == 0 and incomplete[0] == 0 and table[0][0] == rows
    return table[0], np.array(sizes, dtype=np.uint64)


F4_COHORTS = {
    # n = 1, 2 (the unbiased terms' edge), a few odd sizes
    "small": dict(rows=50, cols=37, sizes=(1, 2, 3, 17, 37), seed=1),
    # n up to 70 001: the numerator's cofactors reach 2^33
    "wide": dict(rows=9, cols=70001, sizes=(1, 70001, 35000, 5000, 2), seed=2),
}


@pytest.mark.parametrize("name", list(F4_COHORTS))
def test_f4_against_exact_fractions_every_index_pattern(dev, name):
    slice_, sizes = cohort_table(**F4_COHORTS[name])
    G = len(sizes)
    seen_nan = seen_value = 0
    worst = 0.0
    for A, B, Cc, D in itertools.product(range(G), repeat=4):  # every pattern of repeats among them
        for unbiased in (False, True):
            exact, biased_abs, h_abs = fstat_ref.f4(slice_, sizes, A, B, Cc, D, unbiased)
            got = dev.fstat_f4(slice_, sizes, A, B, Cc, D, unbiased)
            if exact is None:
                assert math.isnan(got), (A, B, Cc, D, unbiased)
                seen_nan += 1
                continue
            bound = (biased_abs + h_abs) / (1 << 50)
            err = abs(Fraction(got) - exact)
            if bound > 0:
                worst = max(worst, float(err / bound))
            assert err <= bound, (A, B, Cc, D, unbiased, got, float(exact), float(err), float(bound))
            seen_value += 1
    print(f"fmh_fstat_f4 {name}: largest error / bound = {worst:.3f}")
    assert seen_nan > 0 and seen_value > 1000  # the one-member group makes NaN wherever its h is needed, and only there


def test_f4_named_statistics_are_index_patterns(dev):
    """f2(A,B) = (A,B;A,B) is the sum of (p_A - p_B)^2 less both bias terms; f3(C;A,B) = (C,A;C,B); checked against direct per-row sums."""
    rng = np.random.default_rng(5)
    rows, cols = 40, 64
    x = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
    masks = np.zeros((3, cols), dtype=bool)
    masks[0, :10], masks[1, 10:33], masks[2, 20:64] = True, True, True
    table, _, _ = fstat_ref.moments(x, None, masks, [(0, rows)])
    sizes = masks.sum(axis=1).astype(np.uint64)
    a, _, _ = fstat_ref.classify(x, None, masks)
    p = [[Fraction(int(a[r, g]), int(sizes[g])) for g in range(3)] for r in range(rows)]
    het = [[p[r][g] * (1 - p[r][g]) / (int(sizes[g]) - 1) for g in range(3)] for r in range(rows)]
    f2 = sum((p[r][0] - p[r][1]) ** 2 - het[r][0] - het[r][1] for r in range(rows))
    f3 = sum((p[r][2] - p[r][0]) * (p[r][2] - p[r][1]) - het[r][2] for r in range(rows))
    f4 = sum((p[r][0] - p[r][1]) * (p[r][2] - p[r][0]) + het[r][0] for r in range(rows))  # A == D adds h_A back
    assert fstat_ref.f4(table[0], sizes, 0, 1, 0, 1, True)[0] == f2
    assert fstat_ref.f4(table[0], sizes, 2, 0, 2, 1, True)[0] == f3
    assert fstat_ref.f4(table[0], sizes, 0, 1, 2, 0, True)[0] == f4
    assert abs(Fraction(dev.fstat_f4(table[0], sizes, 0, 1, 0, 1)) - f2) <= abs(f2) / (1 << 40)
    assert abs(Fraction(dev.fstat_f4(table[0], sizes, 2, 0, 2, 1)) - f3) <= abs(f3) / (1 << 40)


def test_f4_refusals(lib):
    from ferromic_amd import _abi

    table = np.zeros(fstat_ref.moment_count(3), dtype=np.uint64)
    sizes = np.array([4, 5, 6], dtype=np.uint64)
    out = C.c_double()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.fmh_fstat_f4(None, ptr(sizes), 3, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_fstat_f4(ptr(table), None, 3, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_fstat_f4(ptr(table), ptr(sizes), 3, 0, 1, 0, 1, 1, None) == _abi.FMH_ERR_INVALID
    for G in (1, 33):
        assert lib.fmh_fstat_f4(ptr(table), ptr(sizes), G, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_ERR_INVALID
    for bad in ((3, 1, 0, 1), (0, -1, 0, 1), (0, 1, 0, 3)):
        assert lib.fmh_fstat_f4(ptr(table), ptr(sizes), 3, *bad, 1, C.byref(out)) == _abi.FMH_ERR_INVALID
        assert b"outside" in lib.fmh_last_error()
    empty = np.array([4, 0, 6], dtype=np.uint64)
    assert lib.fmh_fstat_f4(ptr(table), ptr(empty), 3, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_fstat_f4(ptr(table), ptr(empty), 3, 0, 2, 0, 2, 1, C.byref(out)) == _abi.FMH_OK  # the empty group is not asked for
    huge = np.array([4, (1 << 17) + 1, 6], dtype=np.uint64)
    assert lib.fmh_fstat_f4(ptr(table), ptr(huge), 3, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_ERR_UNSUPPORTED
    edge = np.array([4, 1 << 17, 6], dtype=np.uint64)
    assert lib.fmh_fstat_f4(ptr(table), ptr(edge), 3, 0, 1, 0, 1, 1, C.byref(out)) == _abi.FMH_OK and out.value == 0.0


# ---- fmh_block_jackknife ------------------------------------------------------------------------------------------------------------------
def test_jackknife_dyadic_blocks_are_exact(dev):
    """Block values for which every f64 operation of the prescribed evaluation is exact (sqrt and the final quotient correctly rounded)."""
    # two equal-weight blocks: theta = 2, theta_(-j) = 3, 1, theta_J = 2, tau = 1, 3, var = 1
    got = dev.block_jackknife([1.0, 3.0], [1.0, 1.0])
    assert got == dict(estimate=2.0, jackknife_estimate=2.0, se=1.0, z=2.0, blocks=2)
    # four: sums less one block are 21, 18, 15, 12 over 3 -> 7, 6, 5, 4; tau = 1, 4, 7, 10; var = (20.25 + 2.25 + 2.25 + 20.25) / 3 / 4
    got = dev.block_jackknife([1.0, 4.0, 7.0, 10.0], [1.0, 1.0, 1.0, 1.0])
    assert got == dict(estimate=5.5, jackknife_estimate=5.5, se=math.sqrt(3.75), z=5.5 / math.sqrt(3.75), blocks=4)
    # unequal weights 1 and 3 (den = weight): theta = 8 / 4 = 2, theta_(-0) = 6 / 3 = 2, theta_(-1) = 2 / 1 = 2 -> no spread at all
    got = dev.block_jackknife([2.0, 6.0], [1.0, 3.0])
    assert got == dict(estimate=2.0, jackknife_estimate=2.0, se=0.0, z=math.inf, blocks=2)
    # unequal den 1 and 3 under explicit weights 2 and 2: theta = 10 / 4 = 2.5, theta_(-0) = 9 / 3 = 3, theta_(-1) = 1 / 1 = 1,
    # theta_J = 5 - (0.5 * 3 + 0.5 * 1) = 3 (not theta: the ratio's bias correction); h = 2, 2; tau = 5 - 3 = 2 and 5 - 1 = 4;
    # var = ((2 - 3)^2 + (4 - 3)^2) / 2 = 1
    got = dev.block_jackknife([1.0, 9.0], [1.0, 3.0], [2.0, 2.0])
    assert got == dict(estimate=2.5, jackknife_estimate=3.0, se=1.0, z=2.5, blocks=2)
    # zero-weight blocks are dropped whatever they hold, in any place
    got = dev.block_jackknife([99.0, 1.0, -5.0, 3.0, 7.0], [5.0, 1.0, 2.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0, 0.0])
    assert got == dict(estimate=2.0, jackknife_estimate=2.0, se=1.0, z=2.0, blocks=2)
    got = dev.block_jackknife([1.0, 8.0, 3.0], [1.0, 0.0, 1.0])  # weight = den: the middle block has none
    assert got == dict(estimate=2.0, jackknife_estimate=2.0, se=1.0, z=2.0, blocks=2)
    for case in (([1.0, 3.0], [1.0, 1.0], None), ([1.0, 4.0, 7.0, 10.0], [1.0] * 4, None), ([1.0, 9.0], [1.0, 3.0], [2.0, 2.0])):
        ref = fstat_ref.jackknife(*case)
        got = dev.block_jackknife(*case)
        assert Fraction(got["estimate"]) == ref["estimate"] and Fraction(got["jackknife_estimate"]) == ref["jackknife_estimate"]
        assert got["se"] == ref["se"] and got["blocks"] == ref["blocks"]


def test_jackknife_degenerate_inputs(dev, lib):
    from ferromic_amd import _abi

    one = dev.block_jackknife([3.0], [4.0])
    assert one["estimate"] == 0.75 and one["jackknife_estimate"] == 0.75 and math.isnan(one["se"]) and math.isnan(one["z"]) and one["blocks"] == 1
    one = dev.block_jackknife([3.0, 5.0, 1.0], [4.0, 9.0, 2.0], [0.0, 0.0, 2.0])  # g = 1 after the zero weights
    assert one["estimate"] == 0.5 and one["jackknife_estimate"] == 0.5 and math.isnan(one["se"]) and one["blocks"] == 1
    for num, den, weight, g in (([1.0, 2.0], [0.0, 0.0], [1.0, 1.0], 2), ([1.0, 2.0], [3.0, -3.0], [1.0, 1.0], 2), ([1.0, 2.0], [0.0, 0.0], None, 0), ([], [], None, 0)):
        got = dev.block_jackknife(num, den, weight)
        assert all(math.isnan(got[k]) for k in ("estimate", "jackknife_estimate", "se", "z")) and got["blocks"] == g, (num, den, weight)
        ref = fstat_ref.jackknife(num, den, weight)
        assert ref["estimate"] is None and ref["blocks"] == g
    out = _abi.JackknifeOut()
    two = (C.c_double * 2)(1.0, 2.0)
    assert lib.fmh_block_jackknife(None, two, None, 2, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_block_jackknife(two, None, None, 2, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_block_jackknife(two, two, None, 2, None) == _abi.FMH_ERR_INVALID
    for bad in (-1.0, math.nan, math.inf):
        weight = (C.c_double * 2)(1.0, bad)
        assert lib.fmh_block_jackknife(two, two, weight, 2, C.byref(out)) == _abi.FMH_ERR_INVALID


def jackknife_cases():
    """Fixed seeds: 2 to 400 blocks of 50 to 5 000 usable rows, per-row means around 0.3, 0.01 and -2 with block-to-block noise; weights =
    the rows, or drawn separately, some of them zero."""
    for seed in range(24):
        rng = np.random.default_rng(1000 + seed)
        g = int(rng.choice([2, 3, 7, 40, 400]))
        den = rng.integers(50, 5000, size=g).astype(np.float64)
        mean = (0.3, 0.01, -2.0)[seed % 3]
        num = den * (mean + rng.normal(0, abs(mean) * 0.2, size=g))
        weight = None
        if seed % 2:
            weight = rng.integers(1, 100, size=g).astype(np.float64)
            if g > 3:
                weight[rng.integers(g)] = 0.0
        yield seed, num, den, weight


def test_jackknife_random_blocks_against_exact_fractions(dev):
    measured = dict.fromkeys(JACKKNIFE_MEASURED, 0.0)
    failures = []
    for seed, num, den, weight in jackknife_cases():
        ref = fstat_ref.jackknife(num, den, weight)
        got = dev.block_jackknife(num, den, weight)
        assert got["blocks"] == ref["blocks"] >= 2
        exact = dict(estimate=ref["estimate"], jackknife_estimate=ref["jackknife_estimate"], se=Fraction(ref["se"]), z=Fraction(ref["z"]))
        for key, want in exact.items():
            deviation = float(abs(Fraction(got[key]) - want) / abs(want))
            measured[key] = max(measured[key], deviation)
            if deviation > JACKKNIFE_MARGIN * JACKKNIFE_MEASURED[key]:
                failures.append((seed, key, deviation))
    print("fmh_block_jackknife: largest relative deviations " + ", ".join(f"{k} = {v:.3e}" for k, v in measured.items()))
    assert not failures, failures


# ---- Python surface: what needs no device ---------------------------------------------------------------------------------------------------
def small_tables():
    rng = np.random.default_rng(9)
    rows, cols = 120, 48
    x = (rng.random((rows, cols)) < rng.beta(0.6, 1.0, size=rows)[:, None]).astype(np.uint8)
    masks = np.zeros((4, cols), dtype=bool)
    masks[0, :9], masks[1, 9:20], masks[2, 20:34], masks[3, 30:48] = True, True, True, True
    blocks = [(0, 30), (30, 55), (55, 55), (55, 120)]
    table, _, _ = fstat_ref.moments(x, None, masks, blocks)
    return table, masks.sum(axis=1).astype(np.uint64), blocks


def test_from_moments_estimates_and_f2_blocks(fm, dev):
    table, sizes, blocks = small_tables()
    s = fm.FStatistics.from_moments(table, [int(n) for n in sizes])
    assert s.moments.dtype == np.uint64 and np.array_equal(s.moments, table) and s.sample_sizes == tuple(int(n) for n in sizes)
    assert s.usable_sites.tolist() == [30, 25, 0, 65] and s.multiallelic_sites.tolist() == [0] * 4 and s.incomplete_sites.tolist() == [0] * 4
    usable = table[:, 0].astype(np.float64)
    for name, args, quad in (("f2", (0, 1), (0, 1, 0, 1)), ("f3", (2, 0, 1), (2, 0, 2, 1)), ("f4", (0, 1, 2, 3), (0, 1, 2, 3)), ("f4", (0, 1, 1, 0), (0, 1, 1, 0))):
        for unbiased in (True, False):
            got = getattr(s, name)(*args, unbiased=unbiased)
            sums = [dev.fstat_f4(table[b], sizes, *quad, unbiased) for b in range(len(blocks))]
            want = dev.block_jackknife(sums, usable)  # the same two C functions, block by block: equal to the bit
            for key in ("estimate", "jackknife_estimate", "se", "z"):
                assert same(getattr(got, key), want[key]), (name, key)
            assert got.blocks == 3 == want["blocks"] and got.sites == 120
            # and the estimate against the exact fractions: the sum of three block sums over 120, each within its own bound
            exact = [fstat_ref.f4(table[b], sizes, *quad, unbiased) for b in range(len(blocks))]
            bound = sum((e[1] + e[2]) for e in exact) / (1 << 50) + 4 * sum(abs(e[0]) for e in exact) / (1 << 53)
            assert abs(Fraction(got.estimate) - sum(e[0] for e in exact) / 120) <= bound / 120 + abs(Fraction(got.estimate)) / (1 << 52)
    assert s.f2(0, 1).estimate == s.f2(0, 1, True).estimate != s.f2(0, 1, unbiased=False).estimate
    ratio = s.f4_ratio((0, 1, 2, 3), (0, 2, 1, 3))
    num = [dev.fstat_f4(table[b], sizes, 0, 1, 2, 3) for b in range(4)]
    den = [dev.fstat_f4(table[b], sizes, 0, 2, 1, 3) for b in range(4)]
    want = dev.block_jackknife(num, den, usable)
    assert ratio.estimate == want["estimate"] and ratio.se == want["se"] and ratio.blocks == 3 and ratio.sites == 120
    # f2_blocks: per-block means [n_blocks][G][G], symmetric, zero diagonal, NaN for the block without a usable row
    f2 = s.f2_blocks()
    assert f2.shape == (4, 4, 4) and f2.dtype == np.float64 and np.isnan(f2[2]).all()
    for b in (0, 1, 3):
        assert np.array_equal(f2[b], f2[b].T) and not f2[b].diagonal().any()
        for i, j in itertools.combinations(range(4), 2):
            exact, biased_abs, h_abs = fstat_ref.f4(table[b], sizes, i, j, i, j, True)
            mean = exact / int(table[b][0])
            # the sum's bound over the rows, and one rounding of the quotient
            assert abs(Fraction(float(f2[b, i, j])) - mean) <= (biased_abs + h_abs) / (1 << 50) / int(table[b][0]) + abs(mean) / (1 << 52), (b, i, j)
    assert not np.array_equal(s.f2_blocks(unbiased=False)[0], f2[0])
    one = fm.FStatistics.from_moments(table[0], [int(n) for n in sizes])  # a single slice is one block
    assert one.moments.shape == (1, 15) and one.f2(0, 1).blocks == 1 and math.isnan(one.f2(0, 1).se) and one.f2(0, 1).estimate == f2[0, 0, 1]


def test_concatenate(fm):
    table, sizes, _ = small_tables()
    sizes = [int(n) for n in sizes]
    a, b = fm.FStatistics.from_moments(table[:1], sizes), fm.FStatistics.from_moments(table[1:], sizes)
    whole = fm.FStatistics.concatenate([a, b])
    assert np.array_equal(whole.moments, table) and whole.sample_sizes == tuple(sizes) and whole.usable_sites.tolist() == [30, 25, 0, 65]
    direct = fm.FStatistics.from_moments(table, sizes)
    for key in ("estimate", "jackknife_estimate", "se", "z", "blocks", "sites"):
        assert same(getattr(whole.f3(2, 0, 1), key), getattr(direct.f3(2, 0, 1), key))
    assert np.array_equal(fm.FStatistics.concatenate([b, a]).moments, np.concatenate([table[1:], table[:1]]))
    assert np.array_equal(fm.FStatistics.concatenate([a]).moments, table[:1])
    other = fm.FStatistics.from_moments(table[:1], sizes[:3] + [sizes[3] + 1])
    with pytest.raises(ValueError):
        fm.FStatistics.concatenate([a, other])
    with pytest.raises(ValueError):
        fm.FStatistics.concatenate([])
    with pytest.raises((ValueError, TypeError)):
        fm.FStatistics.concatenate([a, "b"])


def records(n_sites=4, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


def test_python_surface_and_argument_errors(fm):
    """Every error here is raised before any device use: this test runs where there is no GPU."""
    assert callable(fm.f_statistics)
    for name in ("moments", "sample_sizes", "usable_sites", "multiallelic_sites", "incomplete_sites", "f2", "f3", "f4", "f4_ratio", "f2_blocks",
                 "from_moments", "concatenate"):
        assert hasattr(fm.FStatistics, name), name
    for name in ("estimate", "jackknife_estimate", "se", "z", "blocks", "sites"):
        assert hasattr(fm.FStatEstimate, name), name
    base = fm.Population("s", records(), [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], 100)
    pops = [base.with_haplotypes(g, [(g, 0), (g, 1)]) for g in range(3)]
    with pytest.raises(ValueError) as err:
        fm.f_statistics(pops[:1])
    assert "2 to 32" in str(err.value)
    with pytest.raises(ValueError):
        fm.f_statistics([])
    with pytest.raises(ValueError) as err:
        fm.f_statistics([pops[g % 3] for g in range(33)])
    assert "2 to 32" in str(err.value)
    with pytest.raises(ValueError) as err:
        fm.f_statistics(pops, blocks=[(0, 10)], block_size=10)
    assert "not both" in str(err.value)
    for bad in (0, -5, 2.5, "wide"):
        with pytest.raises(ValueError):
            fm.f_statistics(pops, block_size=bad)
    for bad in ([(1,)], [5], [(1, 2, 3)], [("a", 2)], [(30, 20)]):
        with pytest.raises(ValueError):
            fm.f_statistics(pops, blocks=bad)
    with pytest.raises(ValueError) as err:  # equal variants, another resident matrix: the joint spectrum's rule
        fm.f_statistics([pops[0], fm.Population("t", records(), [(1, 0), (1, 1)], 100)])
    assert "ONE resident matrix" in str(err.value)
    with pytest.raises(ValueError):
        fm.f_statistics([pops[0], base.with_haplotypes(9, [])])  # a population without a haplotype
    with pytest.raises(ValueError):
        fm.f_statistics([pops[0], base.with_haplotypes(9, [(99, 0)])])  # no haplotype is a column of the variants
    with pytest.raises(Exception):
        fm.f_statistics([pops[0], "population"])
    # from_moments: the slice width must be M of the sample sizes
    for moments, sizes in ((np.zeros(6), [3, 4, 5]), (np.zeros((2, 10)), [3, 4]), (np.zeros(6), [3]), (np.zeros(6), [3, 0]), (np.zeros((1, 1, 6)), [3, 4]),
                           (np.zeros(fstat_ref.moment_count(2)), [3] * 33)):
        with pytest.raises((ValueError, TypeError)):
            fm.FStatistics.from_moments(moments, sizes)
    s = fm.FStatistics.from_moments(np.zeros(6, dtype=np.uint64), [3, 4])
    for call in (lambda: s.f2(0, 2), lambda: s.f3(-1, 0, 1), lambda: s.f4(0, 1, 0, 2), lambda: s.f4_ratio((0, 1, 0, 2), (0, 1, 0, 1))):
        with pytest.raises(IndexError):
            call()
    with pytest.raises(ValueError):
        s.f4_ratio((0, 1, 0), (0, 1, 0, 1))
    empty = s.f2(0, 1)
    assert math.isnan(empty.estimate) and empty.blocks == 0 and empty.sites == 0
