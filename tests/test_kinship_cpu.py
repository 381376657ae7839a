"""Relatedness without a GPU: the oracle tests/kinship_ref.py against brute force, fmh_kinship_stats and fmh_kinship_unrelated (host-only
entry points) against the oracle and exact fractions, structural known answers, and the exported names.

Tolerance of the fraction check, u = 2^-53.  Every integer involved is far below 2^53, so the two conversions to f64 are exact; the
division rounds once (error <= u |q|) and, for the kinship, the subtraction from 0.5 rounds once more (error <= u |phi|, of the computed
value, hence the factor 1 + 2u):  |phi - exact| <= u (|q| + |exact|)(1 + 2u),  |distance - exact| <= u |exact|."""

import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import kinship_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = Fraction(1, 2**53)


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


def tiny_cohort(rows, samples, max_allele, missing, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, 2 * samples)) < rng.random((rows, 1))).astype(np.uint8)
    if max_allele > 1:
        high = rng.random(x.shape) < 0.1
        x[high] = rng.integers(2, max_allele + 1, size=int(high.sum()), dtype=np.uint8)
    called = rng.random(x.shape) > 0.15 if missing else None
    return x, called


@pytest.mark.parametrize("max_allele,missing", [(1, False), (1, True), (3, True), (7, False)])
def test_oracle_against_brute_force(max_allele, missing):
    for rows, samples, seed in [(1, 1, 0), (7, 2, 1), (23, 5, 2), (40, 6, 3)]:
        x, called = tiny_cohort(rows, samples, max_allele, missing, seed)
        rng = np.random.default_rng(seed + 100)
        keep = rng.random(rows) < 0.6
        subset = sorted(rng.choice(samples, size=max(1, samples // 2), replace=False).tolist())
        for s, k in [(None, None), (subset, None), (None, keep), (subset, keep)]:
            got = kinship_ref.tables(x, called, s, k)
            ref = kinship_ref.tables_brute(x, called, s, k)
            for a, b in zip(got, ref):
                assert a.dtype == np.uint64 and np.array_equal(a, b), (rows, samples, s is None, k is None)
            both, het_het, ibs0, het_hom = got
            assert np.array_equal(both, both.T) and np.array_equal(het_het, het_het.T) and np.array_equal(ibs0, ibs0.T)
            assert not ibs0.diagonal().any() and not het_hom.diagonal().any()


def stats_cases():
    """(both, het_het, ibs0, het_hom) sets: oracle tables of random cohorts, and hand-made tables with zeros that give NaN."""
    cases = []
    for rows, samples, max_allele, missing, seed in [(60, 6, 1, False, 5), (200, 9, 1, True, 6), (333, 7, 3, True, 7), (90, 4, 7, False, 8)]:
        cases.append(kinship_ref.tables(*tiny_cohort(rows, samples, max_allele, missing, seed)))
    n = 4
    both = np.full((n, n), 10, dtype=np.uint64)
    het_het = np.array([[3, 1, 0, 0], [1, 2, 0, 1], [0, 0, 0, 0], [0, 1, 0, 4]], dtype=np.uint64)
    het_hom = np.array([[0, 2, 3, 0], [1, 0, 2, 1], [0, 0, 0, 0], [4, 3, 4, 0]], dtype=np.uint64)
    ibs0 = np.array([[0, 1, 2, 0], [1, 0, 0, 3], [2, 0, 0, 1], [0, 3, 1, 0]], dtype=np.uint64)
    both[2, 3] = both[3, 2] = 0  # a pair with no common call
    both[2, 2] = 0
    cases.append((both, het_het, ibs0, het_hom))
    return cases


def test_stats_bitwise_against_the_oracle_and_fractions(dev):
    nan_phi = nan_dist = 0
    for both, het_het, ibs0, het_hom in stats_cases():
        phi, dist = dev.kinship_stats(both, het_het, ibs0, het_hom)
        ref_phi, ref_dist = kinship_ref.stats(both, het_het, ibs0, het_hom)
        assert phi.dtype == np.float64 and np.array_equal(phi, ref_phi, equal_nan=True)
        assert np.array_equal(dist, ref_dist, equal_nan=True)
        # the bit patterns too (a NaN is a quiet NaN either way, so compare where finite)
        assert np.array_equal(phi[np.isfinite(phi)].view(np.uint64), ref_phi[np.isfinite(ref_phi)].view(np.uint64))
        only_phi, none = dev.kinship_stats(both, het_het, ibs0, het_hom, ibs_distance=False)
        assert none is None and np.array_equal(only_phi, phi, equal_nan=True)
        n = both.shape[0]
        for i in range(n):
            for j in range(n):
                hom = int(het_hom[i, j]) + int(het_hom[j, i])
                m = min(int(het_het[i, j]) + int(het_hom[i, j]), int(het_het[i, j]) + int(het_hom[j, i]))
                if m == 0:
                    assert math.isnan(phi[i, j])
                    nan_phi += 1
                else:
                    q = Fraction(hom + 4 * int(ibs0[i, j]), 4 * m)
                    exact = Fraction(1, 2) - q
                    assert abs(Fraction(float(phi[i, j])) - exact) <= U * (abs(q) + abs(exact)) * (1 + 2 * U), (i, j)
                if both[i, j] == 0:
                    assert math.isnan(dist[i, j])
                    nan_dist += 1
                else:
                    exact = Fraction(hom + 2 * int(ibs0[i, j]), 2 * int(both[i, j]))
                    assert abs(Fraction(float(dist[i, j])) - exact) <= U * abs(exact), (i, j)
                if i == j and m:
                    assert phi[i, j] == 0.5
    assert nan_phi > 0 and nan_dist > 0  # both NaN rules were met


def test_stats_refusals(lib):
    from ferromic_amd import _abi

    t = np.ones((2, 2), dtype=np.uint64)
    out = np.zeros((2, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.fmh_kinship_stats(p(t), p(t), p(t), p(t), 2, p(out), None) == 0
    for k in range(5):
        args = [p(t), p(t), p(t), p(t), 2, p(out), None]
        args[k if k < 4 else 5] = None
        assert lib.fmh_kinship_stats(*args) == _abi.FMH_ERR_INVALID
    assert lib.fmh_kinship_stats(None, None, None, None, 0, None, None) == 0
    keep = np.zeros(2, dtype=np.uint8)
    assert lib.fmh_kinship_unrelated(None, 2, 0.1, p(keep)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_kinship_unrelated(p(out), 2, 0.1, None) == _abi.FMH_ERR_INVALID
    assert lib.fmh_kinship_unrelated(None, 0, 0.1, None) == 0


def test_unrelated_against_the_python_rule(dev):
    nan = float("nan")
    # a chain 0-1-2-3: the ends have one partner, the middle two: tie between 1 and 2 -> the higher index goes first, then 0-1 remains
    chain = np.zeros((4, 4))
    for i, j in [(0, 1), (1, 2), (2, 3)]:
        chain[i, j] = chain[j, i] = 0.3
    np.fill_diagonal(chain, 0.5)
    got = dev.kinship_unrelated(chain, 0.1)
    assert got.tolist() == kinship_ref.unrelated(chain, 0.1).tolist() == [True, False, False, True]
    # a star: the hub goes, the leaves stay
    star = np.zeros((5, 5))
    star[0, 1:] = star[1:, 0] = 0.26
    assert dev.kinship_unrelated(star, 0.25).tolist() == [False, True, True, True, True]
    # a threshold that nothing exceeds; the diagonal (0.5) is no pair
    assert dev.kinship_unrelated(star, 0.26).all() and dev.kinship_unrelated(chain, 0.3).all()
    # NaN never exceeds
    with_nan = chain.copy()
    with_nan[1, 2] = with_nan[2, 1] = nan
    assert dev.kinship_unrelated(with_nan, 0.1).tolist() == kinship_ref.unrelated(with_nan, 0.1).tolist() == [True, False, True, False]
    assert dev.kinship_unrelated(np.full((3, 3), nan), 0.0).all()
    # random symmetric matrices with ties (few distinct values) and NaNs, several thresholds
    rng = np.random.default_rng(12)
    removed = 0
    for n in (1, 2, 7, 20, 41):
        for _ in range(6):
            upper = np.triu(rng.choice([0.0, 0.05, 0.12, 0.25, 0.5, nan], size=(n, n), p=[0.5, 0.2, 0.1, 0.1, 0.05, 0.05]), 1)
            phi = upper + upper.T
            np.fill_diagonal(phi, 0.5)
            for threshold in (-1.0, 0.0, 0.04, 0.0884, 0.2, 0.5):
                got = dev.kinship_unrelated(phi, threshold)
                ref = kinship_ref.unrelated(phi, threshold)
                assert got.dtype == bool and got.tolist() == ref.tolist(), (n, threshold)
                left = phi[np.ix_(got, got)].copy()
                np.fill_diagonal(left, np.nan)
                assert not (left > threshold).any()
                removed += int((~got).sum())
    assert removed > 0


def related_cohort(rows=3000, founders=12, seed=21):
    """Founders with independent genotypes; sample `founders` duplicates founder 0; sample founders + 1 is a child of founder 1 and founder 2
    (one allele of each, picked at random per site).  Columns: 2 s, 2 s + 1 of sample s."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.95, size=(rows, 1))
    x = (rng.random((rows, 2 * founders)) < freq).astype(np.uint8)
    dup = x[:, 0:2]
    pick1 = rng.integers(0, 2, size=rows)
    pick2 = rng.integers(0, 2, size=rows)
    child = np.stack([x[np.arange(rows), 2 + pick1], x[np.arange(rows), 4 + pick2]], axis=1)
    return np.concatenate([x, dup, child], axis=1), founders, founders + 1


def test_structural_known_answers(dev):
    x, dup, child = related_cohort()
    both, het_het, ibs0, het_hom = kinship_ref.tables(x, None)
    phi, dist = dev.kinship_stats(both, het_het, ibs0, het_hom)
    assert phi[0, dup] == 0.5 and phi[dup, 0] == 0.5 and dist[0, dup] == 0.0  # a duplicated sample: exactly one half
    assert ibs0[1, child] == 0 and ibs0[2, child] == 0 and ibs0[child, 1] == 0  # parent and offspring share an allele at every site
    unrelated_pairs = [phi[i, j] for i in range(3, dup) for j in range(i + 1, dup)]
    assert phi[0, dup] > phi[1, child] > max(unrelated_pairs)
    assert phi[0, dup] > phi[2, child] > max(unrelated_pairs)
    assert abs(phi[1, child] - 0.25) < 0.05 and max(abs(v) for v in unrelated_pairs) < 0.1  # 3 000 independent sites
    assert np.array_equal(phi, phi.T) and (phi.diagonal() == 0.5).all()
    # the greedy rule at the usual second-degree cutoff removes one of each related pair / trio and nobody else
    keep = dev.kinship_unrelated(phi, 0.0884)
    assert keep.tolist() == kinship_ref.unrelated(phi, 0.0884).tolist()
    assert keep[3:dup].all() and not (keep[0] and keep[dup]) and not keep[child] and keep[1] and keep[2]


def test_symbols_and_option_are_exported(lib):
    from ferromic_amd import _abi

    for name in ("fmh_kinship_counts", "fmh_kinship_stats", "fmh_kinship_unrelated"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
    assert _abi.get_option("FMH_KIN_BUDGET_BYTES") == 16 << 30
    import ferromic

    assert ferromic.Kinship.__module__.endswith("_core") and callable(ferromic.kinship)
    assert hasattr(ferromic.Population, "kinship")
