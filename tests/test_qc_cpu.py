"""Genotype QC without a GPU: the oracle of tests/qc_ref.py against brute force, and the library's host functions (fmh_hwe_exact_host,
fmh_genotype_site_stats, fmh_genotype_site_weights, fmh_genotype_sample_stats, the filters of ferromic.GenotypeQC) against it - bitwise -
and against exact fractions.Fraction arithmetic.

The exact test's tolerance against the fractions is measured, not assumed: the worst relative error of the seeded set below (the 12 341
triples with N <= 40 and 400 random ones at N = 100, 257, 1 000, 2 500) is 3.061e-15; sixteen times that is asserted."""

import math
from fractions import Fraction

import numpy as np
import pytest

from tests import qc_ref

HWE_WORST_REL = 3.061e-15  # measured on this file's seeded set
HWE_TOL = 16 * HWE_WORST_REL


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(got, ref, what):
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok]), (what, np.flatnonzero(bits(got) != bits(ref))[:4].tolist())


# ---- the oracle itself ------------------------------------------------------------------------------------------------------------------
def small_cohort(seed, rows=23, samples=9, max_allele=3, missing=True):
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, 2 * samples)) < 0.4).astype(np.uint8)
    high = rng.random(x.shape) < 0.05
    x[high] = rng.integers(2, max_allele + 1, size=int(high.sum()), dtype=np.uint8)
    called = rng.random(x.shape) > 0.1 if missing else None
    return x, called


@pytest.mark.parametrize("missing", [False, True])
def test_oracle_against_brute_force(missing):
    x, called = small_cohort(3, missing=missing)
    rng = np.random.default_rng(4)
    weights = rng.integers(0, 1 << 32, size=x.shape[0], dtype=np.uint64).astype(np.uint32)
    weights[:4] = [0, 1, 1 << 31, (1 << 32) - 1]
    for samples in (None, [0, 3, 4, 8]):
        for keep in (None, rng.random(x.shape[0]) < 0.5):
            site, sample, weighted = qc_ref.counts_brute(x, called, samples, keep, weights)
            for got, ref in zip(qc_ref.site_tracks(x, called, samples), site):
                assert got.dtype == np.uint32 and np.array_equal(got, ref)
            for got, ref in zip(qc_ref.sample_tables(x, called, samples, keep), sample):
                assert got.dtype == np.uint64 and np.array_equal(got, ref)
            assert np.array_equal(qc_ref.weighted_called(x, called, weights, samples, keep), weighted)
    # the classes partition the called genotypes, an upper allele un-calls a genotype, the tracks ignore the keep mask
    c, g = qc_ref.classes(x, called)
    assert sum(t.astype(np.int64) for t in qc_ref.site_tracks(x, called)).tolist() == c.sum(axis=1).tolist()
    assert (c.sum(axis=1) < x.shape[1] // 2).any()


# ---- the exact test -----------------------------------------------------------------------------------------------------------------------
def all_triples(max_n):
    """(hom_ref, het, hom_alt) with N <= max_n."""
    return np.array([(a, b, N - a - b) for N in range(max_n + 1) for a in range(N + 1) for b in range(N + 1 - a)], dtype=np.uint32)


def seeded_triples():
    rng = np.random.default_rng(2005)
    out = []
    for N in (100, 257, 1000, 2500):
        for _ in range(100):
            a = int(rng.integers(0, N + 1))
            b = int(rng.integers(0, N + 1 - a))
            out.append((a, b, N - a - b))
    return np.array(out, dtype=np.uint32)


# in the order (hom_ref, het, hom_alt): N = 0; monomorphic both ways; rare = 1 and 2; all het; the two underflows (no het of 2 500 at
# p = 0.5, and 2 500 hets of 2 500)
SPECIAL = np.array([(0, 0, 0), (7, 0, 0), (0, 0, 2500), (9, 1, 0), (0, 1, 9), (9, 2, 0), (9, 0, 1), (1, 0, 9), (1, 1, 0), (0, 5, 0),
                    (1250, 0, 1250), (0, 2500, 0)], dtype=np.uint32)


def test_hwe_host_is_the_python_loop_bit_for_bit(dev):
    for name, t in (("N <= 40", all_triples(40)), ("seeded", seeded_triples()), ("special", SPECIAL)):
        got = dev.hwe_exact_host(t[:, 0], t[:, 1], t[:, 2])
        assert_bitwise(got, qc_ref.hwe(t[:, 0], t[:, 1], t[:, 2]), name)
        swapped = dev.hwe_exact_host(t[:, 2], t[:, 1], t[:, 0])
        assert_bitwise(swapped, got, name + ", hom_ref and hom_alt swapped")
        finite = got[~np.isnan(got)]
        assert ((finite >= 0.0) & (finite <= 1.0)).all(), name


def test_hwe_special_cases(dev):
    got = dev.hwe_exact_host(SPECIAL[:, 0], SPECIAL[:, 1], SPECIAL[:, 2])
    assert math.isnan(got[0])
    assert got[1] == 1.0 and got[2] == 1.0            # monomorphic
    assert got[3] == 1.0 and got[4] == 1.0            # rare = 1: one possible het count
    assert got[5] == 1.0 and 0.0 < got[6] < 1.0       # rare = 2: het = 2 is the mode, het = 0 the rarer table
    assert got[6] == got[7]
    assert bits(got[10:])[0] == 0 and bits(got[10:])[1] == 0   # exactly +0.0
    assert dev.hwe_exact_host([], [], []).size == 0


def test_hwe_refuses_more_than_2_26_genotypes(dev):
    from ferromic_amd import _abi

    big = (1 << 26) + 1
    with pytest.raises(_abi.FerromicHipError):
        dev.hwe_exact_host([big], [0], [0])
    assert dev.hwe_exact_host([1 << 26], [0], [0])[0] == 1.0
    assert math.isnan(qc_ref.hwe_p(big, 0, 0))


def test_hwe_host_against_exact_fractions(dev):
    worst = 0.0
    for t in (all_triples(40), seeded_triples(), SPECIAL):
        got = dev.hwe_exact_host(t[:, 0], t[:, 1], t[:, 2])
        for (a, b, c), g in zip(t.tolist(), got.tolist()):
            if a + b + c == 0:
                continue
            exact = qc_ref.hwe_exact_fraction(a, b, c)
            if exact >= Fraction(1, 10**290):
                rel = abs(float(Fraction(g) / exact - 1))
                worst = max(worst, rel)
                assert rel <= HWE_TOL, (a, b, c, g, float(exact), rel)
            else:
                assert g <= 1e-280, (a, b, c, g)
    print(f"worst relative error against the exact fractions: {worst:.3e} (asserted: {HWE_TOL:.3e})")


# ---- the estimators -------------------------------------------------------------------------------------------------------------------------
def one_rounding(got, exact_ops):
    """|got - exact| within `exact_ops` roundings of the exact value (a Fraction)."""
    if exact_ops[0] == 0:
        return got == 0.0
    return abs(Fraction(got) / exact_ops[0] - 1) <= exact_ops[1] * Fraction(1, 2**53) * Fraction(101, 100)


def test_site_stats_and_weights(dev):
    t = np.concatenate([all_triples(12), seeded_triples(), np.array([(0, 0, 0), (5, 0, 0), (0, 0, 5), (0, 1, 0), (1, 0, 0)], dtype=np.uint32)])
    n = int(t.sum(axis=1).max()) + 3
    got = dev.genotype_site_stats(t[:, 0], t[:, 1], t[:, 2], n)
    ref = qc_ref.site_stats(t[:, 0], t[:, 1], t[:, 2], n)
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert_bitwise(got[name], ref[name], name)
    w = dev.genotype_site_weights(t[:, 0], t[:, 1], t[:, 2])
    assert w.dtype == np.uint32 and np.array_equal(w, qc_ref.site_weights(t[:, 0], t[:, 1], t[:, 2]))
    assert w.max() == 1 << 31 and w.min() == 0   # N = 1, het: e = 1; monomorphic: e = 0
    for (a, b, c), i in zip(t.tolist(), range(len(t))):
        N, n_alt = a + b + c, 2 * c + b
        n_ref = 2 * N - n_alt
        if N == 0:
            assert all(math.isnan(got[k][i]) for k in ("alt_frequency", "maf", "f_is", "expected_het")) and got["call_rate"][i] == 0.0 and w[i] == 0
            continue
        p = Fraction(n_alt, 2 * N)
        assert one_rounding(got["call_rate"][i], (Fraction(N, n), 1))
        assert one_rounding(got["alt_frequency"][i], (p, 1))
        assert abs(Fraction(got["maf"][i]) - min(p, 1 - p)) <= 2 * Fraction(1, 2**53)   # p, then 1 - p: values of at most 1
        assert one_rounding(got["expected_het"][i], (Fraction(n_alt * n_ref, 2 * N - 1), 1))
        if n_alt * n_ref == 0:
            assert math.isnan(got["f_is"][i])
        else:  # 1 - q: the rounding of q, then of the difference, both relative to values of at most max(1, q)
            q = Fraction(b * (2 * N - 1), n_alt * n_ref)
            assert abs(Fraction(got["f_is"][i]) - (1 - q)) <= 2 * max(1, q) * Fraction(1, 2**53)
        e = Fraction(n_alt * n_ref, N * (2 * N - 1))
        assert abs(int(w[i]) - e * 2**31) <= Fraction(1, 2) + Fraction(1, 2**20)   # rint of a value one rounding from exact
    # the counts of a u64 product: a site with 2^31 genotypes is refused
    from ferromic_amd import _abi

    with pytest.raises(_abi.FerromicHipError):
        dev.genotype_site_stats([1 << 31], [0], [0], 1 << 31)
    with pytest.raises(_abi.FerromicHipError):
        dev.genotype_site_weights([1 << 30], [1 << 30], [0])


def test_sample_stats(dev):
    rng = np.random.default_rng(8)
    n, kept = 50, 1000
    het = rng.integers(0, 400, size=n).astype(np.uint64)
    hom_ref = rng.integers(0, 400, size=n).astype(np.uint64)
    hom_alt = rng.integers(0, 200, size=n).astype(np.uint64)
    weighted = (rng.random(n) * 300 * 2**31).astype(np.uint64) + np.uint64(1)
    het[0] = hom_ref[0] = hom_alt[0] = 0   # a sample without a call
    weighted[0] = 0
    weighted[1] = (1 << 63) + 12345        # above 2^53: the conversion rounds, as numpy's does
    got = dev.genotype_sample_stats(hom_ref, het, hom_alt, kept, weighted)
    ref = qc_ref.sample_stats(hom_ref, het, hom_alt, kept, weighted)
    assert sorted(got) == ["call_rate", "f", "het_rate"]
    for name in ref:
        assert_bitwise(got[name], ref[name], name)
    assert math.isnan(got["het_rate"][0]) and math.isnan(got["f"][0]) and got["call_rate"][0] == 0.0
    for i in range(2, n):
        called = int(hom_ref[i] + het[i] + hom_alt[i])
        assert one_rounding(got["call_rate"][i], (Fraction(called, kept), 1))
        assert one_rounding(got["het_rate"][i], (Fraction(int(het[i]), called), 1))
        q = Fraction(int(het[i]) * 2**31, int(weighted[i]))
        assert abs(Fraction(got["f"][i]) - (1 - q)) <= 3 * max(1, q) * Fraction(1, 2**53)
    without = dev.genotype_sample_stats(hom_ref, het, hom_alt, 0)
    assert sorted(without) == ["call_rate", "het_rate"] and np.isnan(without["call_rate"]).all()
    assert_bitwise(without["het_rate"], ref["het_rate"], "het_rate without weights")


# ---- the filters of the Python result: only the criteria given, a NaN fails a criterion it is tested on ---------------------------------------
def test_filters_nan_rule():
    import ferromic

    # sites: complete and in HWE; no call at all (every statistic NaN but call_rate 0); monomorphic (maf 0, hwe 1); all het (hwe small)
    hom_ref = np.array([5, 0, 20, 0], dtype=np.uint32)
    het = np.array([10, 0, 0, 20], dtype=np.uint32)
    hom_alt = np.array([5, 0, 0, 0], dtype=np.uint32)
    # samples: called everywhere; never called (het_rate and F NaN); half called
    s_ref = np.array([2, 0, 1], dtype=np.uint64)
    s_het = np.array([1, 0, 1], dtype=np.uint64)
    s_alt = np.array([1, 0, 0], dtype=np.uint64)
    weighted = np.array([2 << 31, 0, 1 << 31], dtype=np.uint64)
    qc = ferromic.GenotypeQC.from_counts(hom_ref, het, hom_alt, 20, s_ref, s_het, s_alt, 4, weighted)
    assert np.array_equal(qc.hom_ref, hom_ref) and qc.hom_ref.dtype == np.uint32 and qc.sample_het.dtype == np.uint64
    ref = qc_ref.site_stats(hom_ref, het, hom_alt, 20)
    for name in ("call_rate", "alt_frequency", "maf", "f_is"):
        assert_bitwise(getattr(qc, name), ref[name], name)
    assert_bitwise(qc.hwe_p, qc_ref.hwe(hom_ref, het, hom_alt), "hwe_p")
    sref = qc_ref.sample_stats(s_ref, s_het, s_alt, 4, weighted)
    assert_bitwise(qc.sample_call_rate, sref["call_rate"], "sample_call_rate")
    assert_bitwise(qc.sample_het_rate, sref["het_rate"], "sample_het_rate")
    assert_bitwise(qc.sample_f, sref["f"], "sample_f")
    assert math.isnan(qc.maf[1]) and math.isnan(qc.hwe_p[1]) and math.isnan(qc.sample_f[1])

    assert qc.site_filter().tolist() == [True, True, True, True]          # no criterion: nothing is tested, not even a NaN
    assert qc.site_filter(min_call_rate=0.5).tolist() == [True, False, True, True]
    assert qc.site_filter(min_maf=0.0).tolist() == [True, False, True, True]       # NaN fails the criterion it is tested on
    assert qc.site_filter(min_maf=0.01).tolist() == [True, False, False, True]
    assert qc.site_filter(min_hwe_p=1e-3).tolist() == [True, False, True, False]
    assert qc.site_filter(min_call_rate=0.0, min_hwe_p=0.0).tolist() == [True, False, True, True]
    assert qc.site_filter(min_call_rate=1.0, min_maf=0.3, min_hwe_p=0.5).tolist() == [True, False, False, False]
    assert qc.site_filter().dtype == bool
    assert qc.sample_filter().tolist() == [True, True, True]
    assert qc.sample_filter(min_call_rate=0.5).tolist() == [True, False, True]
    assert qc.sample_filter(max_abs_f=10.0).tolist() == [True, False, True]
    f = qc.sample_f
    assert qc.sample_filter(max_abs_f=abs(f[0])).tolist() == [True, False, abs(f[2]) <= abs(f[0])]
    assert qc.sample_filter(min_call_rate=0.9, max_abs_f=10.0).tolist() == [True, False, False]
    # without the weighted sums there is no F: testing it is an error, not a silent pass
    bare = ferromic.GenotypeQC.from_counts(hom_ref, het, hom_alt, 20, s_ref, s_het, s_alt, 4)
    assert bare.sample_f is None
    with pytest.raises(ValueError):
        bare.sample_filter(max_abs_f=0.1)
