"""Site frequency spectra without a GPU: the exported symbols and their prototypes, the refusals that need no device, fmh_sfs_stats
against the plain-Python formulas of tests/sfs_ref.py, and the Python surface (SiteFrequencySpectrum.from_counts, folded(), per-window
shapes, argument errors raised before any device use).

Tolerances are derived, not chosen.  With u = 2^-53:
  * pi_sum, theta_w_sum and theta_h_sum are sums of at most n non-negative terms (theta_w through a1 = sum 1/i).  A term costs at most three
    roundings (products, quotient) and the running sum one per term, so a straightforward f64 evaluation is within (n + 3) u relative of the
    true value - there is no cancellation.  Two such evaluations differ by at most 2 (n + 3) u < (n + 4) 2^-52 relative: the bound used
    for the three sums.  (The oracle sums with math.fsum, so in practice half of it is unused.)
  * Tajima's D = (pi_sum - theta_w_sum) / sd.  The numerator is a difference of two quantities each within the bound above, so its absolute
    error is at most (n + 4) 2^-52 (pi_sum + theta_w_sum); divided by sd that bounds the error of D.  sd's own relative error (a1 and a2 are
    sums of positive terms, c1 and c2 lose no more than a digit) scales D, and |D| <= (pi_sum + theta_w_sum) / sd, so it is covered by the
    half of the bound the oracle's exact sums leave unused.
"""

import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import sfs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import _abi

    return _abi.load()


@pytest.fixture(scope="module")
def fm(lib):
    import ferromic

    return ferromic


def test_symbols_are_exported_and_prototyped(lib):
    from ferromic_amd import _abi

    for name, n_args in (("fmh_sfs", 7), ("fmh_sfs_joint", 7), ("fmh_sfs_stats", 3)):
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_abi.SfsSkipped) == 16 and C.sizeof(_abi.SfsStatsOut) == 7 * 8
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    assert "#define FMH_ABI_VERSION 3" in header and "fmh_sfs_skipped" in header and "fmh_sfs_stats_out" in header
    for key in ("FMH_SFS_ITEM_ROWS", "FMH_SFS_LDS_BINS"):
        assert _abi.get_option(key) == 0 and key in header
        _abi.set_option(key, 7)
        assert _abi.get_option(key) == 7
        _abi.set_option(key, None)
        assert _abi.get_option(key) == 0


def test_null_arguments_are_refused_without_a_device(lib):
    from ferromic_amd import _abi

    table = np.zeros(4, dtype=np.uint64)
    windows = np.array([0, 0], dtype=np.uint64)
    t, w = table.ctypes.data_as(C.c_void_p), windows.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)  # never dereferenced: the NULL argument is found first
    assert lib.fmh_sfs(None, None, w, 1, t, None, None) == _abi.FMH_ERR_INVALID
    assert b"NULL matrix" in lib.fmh_last_error()
    assert lib.fmh_sfs_joint(None, None, 0, 0, t, None, None) == _abi.FMH_ERR_INVALID
    assert b"NULL matrix" in lib.fmh_last_error()
    assert lib.fmh_sfs(fake, None, w, 1, t, None, None) == _abi.FMH_ERR_INVALID
    assert b"NULL groups" in lib.fmh_last_error()
    assert lib.fmh_sfs_joint(fake, None, 0, 0, t, None, None) == _abi.FMH_ERR_INVALID
    assert b"NULL groups" in lib.fmh_last_error()
    assert lib.fmh_sfs(fake, fake, w, 1, None, None, None) == _abi.FMH_ERR_INVALID
    assert b"d_sfs" in lib.fmh_last_error()
    assert lib.fmh_sfs_joint(fake, fake, 0, 0, None, None, None) == _abi.FMH_ERR_INVALID
    assert lib.fmh_sfs(fake, fake, None, 1, t, None, None) == _abi.FMH_ERR_INVALID
    assert b"h_windows" in lib.fmh_last_error()
    out = _abi.SfsStatsOut()
    assert lib.fmh_sfs_stats(None, 3, C.byref(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_sfs_stats(t, 3, None) == _abi.FMH_ERR_INVALID


# ---- fmh_sfs_stats ---------------------------------------------------------------------------------------------------------------------
def sum_bound(n):
    return (n + 4) * 2.0 ** -52


def check_stats(counts):
    from ferromic_amd import device

    got = device.sfs_stats(counts)
    ref = sfs_ref.stats(counts)
    n = len(counts) - 1
    assert got["sites"] == ref["sites"] and got["segregating_sites"] == ref["segregating_sites"]
    for key in ("pi_sum", "theta_w_sum", "theta_h_sum"):
        if math.isnan(ref[key]):
            assert math.isnan(got[key]), key
        else:
            assert abs(got[key] - ref[key]) <= sum_bound(n) * abs(ref[key]), (key, got[key], ref[key])
    if math.isnan(ref["fay_wu_h"]):
        assert math.isnan(got["fay_wu_h"])
    else:  # a difference of two sums, each within the bound
        assert abs(got["fay_wu_h"] - ref["fay_wu_h"]) <= sum_bound(n) * (ref["pi_sum"] + ref["theta_h_sum"])
    if math.isnan(ref["tajima_d"]):
        assert math.isnan(got["tajima_d"])
    else:
        bound = sum_bound(n) * (ref["pi_sum"] + ref["theta_w_sum"]) / ref["tajima_d_sd"]
        print(f"n={n} D={got['tajima_d']!r} ref={ref['tajima_d']!r} |diff|={abs(got['tajima_d'] - ref['tajima_d']):.3e} bound={bound:.3e}")
        assert abs(got["tajima_d"] - ref["tajima_d"]) <= bound, (got["tajima_d"], ref["tajima_d"], bound)
    return got


def test_stats_known_answer_tajima_worked_example(lib):
    """n = 10, S = 16, pi = 3.888...: the worked example of Tajima's D, here in f64."""
    counts = [0, 13, 1, 2, 0, 0, 0, 0, 0, 0, 0]
    got = check_stats(counts)
    n = 10
    assert got["sites"] == 16 and got["segregating_sites"] == 16
    for key, value in (("pi_sum", 3.888888888888889), ("theta_w_sum", 5.655772198064245), ("theta_h_sum", 0.7777777777777778)):
        assert abs(got[key] - value) <= sum_bound(n) * value, key
    ref = sfs_ref.stats(counts)
    assert abs(got["tajima_d"] - -1.446172076557919) <= sum_bound(n) * (3.888888888888889 + 5.655772198064245) / ref["tajima_d_sd"]
    assert abs(ref["tajima_d"] - -1.446172076557919) <= 1e-15
    assert abs(got["fay_wu_h"] - (3.888888888888889 - 0.7777777777777778)) <= sum_bound(n) * 5.0


def test_stats_small_samples(lib):
    from ferromic_amd import device

    for n in (2, 3):  # the variance is zero on paper: D is NaN by rule, the sums are not
        counts = [0] * (n + 1)
        counts[1] = 3
        got = check_stats(counts)
        assert math.isnan(got["tajima_d"]) and got["segregating_sites"] == 3 and got["pi_sum"] > 0
    got = check_stats([0, 3, 0, 0, 0])  # n = 4, three singletons
    assert abs(got["tajima_d"] - -0.7544510776527732) <= sum_bound(4) * (got["pi_sum"] + got["theta_w_sum"]) / sfs_ref.stats([0, 3, 0, 0, 0])["tajima_d_sd"]
    for n in (2, 4, 11):  # all bins zero
        got = check_stats([0] * (n + 1))
        assert math.isnan(got["tajima_d"]) and got["pi_sum"] == 0.0 and got["theta_w_sum"] == 0.0 and got["theta_h_sum"] == 0.0
    got = check_stats([5, 0, 7])  # monomorphic rows only
    assert got["sites"] == 12 and got["segregating_sites"] == 0 and math.isnan(got["tajima_d"])
    for counts in ([4, 9], [6]):  # n = 1 and n = 0: every f64 field NaN
        got = device.sfs_stats(counts)
        assert got["sites"] == sum(counts) and got["segregating_sites"] == 0
        assert all(math.isnan(got[k]) for k in ("pi_sum", "theta_w_sum", "theta_h_sum", "tajima_d", "fay_wu_h"))


@pytest.mark.parametrize("n", [4, 5, 64, 5000])
def test_stats_random_spectra(lib, n):
    rng = np.random.default_rng(n)
    for trial in range(4):
        weights = 1.0 / np.arange(1, n + 2) if trial % 2 == 0 else np.ones(n + 1)
        counts = rng.poisson(weights * rng.choice([3.0, 1e3, 1e7]))
        counts[0] += 100
        if not counts[1:n].any():
            counts[1] = 1
        check_stats([int(c) for c in counts])
    big = [0] * (n + 1)
    big[n // 2] = 2**40  # counts far beyond 2^32
    big[1] = 3
    check_stats(big)


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def test_from_counts_statistics_and_folding(fm):
    even = [7, 13, 1, 2, 0, 0, 5, 0, 0, 3, 11]  # n = 10
    s = fm.SiteFrequencySpectrum.from_counts(even)
    assert s.sample_size == 10 and s.counts.dtype == np.uint64 and s.counts.tolist() == even
    assert s.multiallelic_sites == 0 and s.incomplete_sites == 0
    assert s.folded().tolist() == sfs_ref.folded(even) == [18, 16, 1, 2, 5, 0] and s.folded().dtype == np.uint64
    ref = sfs_ref.stats(even)
    assert s.segregating_sites == ref["segregating_sites"] and isinstance(s.theta_pi, float)
    for got, key in ((s.theta_pi, "pi_sum"), (s.theta_w, "theta_w_sum"), (s.theta_h, "theta_h_sum")):
        assert abs(got - ref[key]) <= sum_bound(10) * ref[key]
    assert abs(s.tajimas_d - ref["tajima_d"]) <= sum_bound(10) * (ref["pi_sum"] + ref["theta_w_sum"]) / ref["tajima_d_sd"]
    assert abs(s.fay_wu_h - ref["fay_wu_h"]) <= sum_bound(10) * (ref["pi_sum"] + ref["theta_h_sum"])
    odd = [1, 2, 3, 4, 5, 6]  # n = 5: no middle bin
    assert fm.SiteFrequencySpectrum.from_counts(odd).folded().tolist() == sfs_ref.folded(odd) == [7, 7, 7]
    assert fm.SiteFrequencySpectrum.from_counts(np.array([4, 9], dtype=np.int32)).folded().tolist() == [13]


def test_from_counts_per_window_shapes(fm):
    table = np.array([[0, 3, 0, 0, 0], [1, 2, 3, 4, 5], [9, 0, 0, 0, 9]], dtype=np.uint64)
    s = fm.SiteFrequencySpectrum.from_counts(table)
    assert s.sample_size == 4 and s.counts.shape == (3, 5) and np.array_equal(s.counts, table)
    assert s.folded().shape == (3, 3) and s.folded().tolist() == [sfs_ref.folded(r) for r in table]
    assert s.segregating_sites.tolist() == [3, 9, 0] and s.multiallelic_sites.tolist() == [0, 0, 0] and s.incomplete_sites.shape == (3,)
    for name in ("theta_pi", "theta_w", "theta_h", "tajimas_d", "fay_wu_h"):
        value = getattr(s, name)
        assert isinstance(value, np.ndarray) and value.dtype == np.float64 and value.shape == (3,), name
        for w in range(3):
            one = getattr(fm.SiteFrequencySpectrum.from_counts(table[w]), name)
            assert value[w] == one or (math.isnan(value[w]) and math.isnan(one)), (name, w)
    assert math.isnan(s.tajimas_d[2]) and s.tajimas_d[0] == fm.SiteFrequencySpectrum.from_counts([0, 3, 0, 0, 0]).tajimas_d
    for bad in ([], [3], np.zeros((2, 2, 2)), "spectrum"):
        with pytest.raises((ValueError, TypeError)):
            fm.SiteFrequencySpectrum.from_counts(bad)


def records(n_sites=4, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


def test_python_surface_and_argument_errors(fm):
    """Every error here is raised before any device use: this test runs where there is no GPU."""
    assert callable(fm.site_frequency_spectrum) and callable(fm.joint_site_frequency_spectrum)
    assert callable(fm.Population.site_frequency_spectrum) and hasattr(fm.JointSiteFrequencySpectrum, "marginal")
    two = [(0, 0), (0, 1)]
    with pytest.raises(ValueError):
        fm.site_frequency_spectrum(records(), [])  # too few haplotypes
    with pytest.raises(ValueError):
        fm.site_frequency_spectrum(records(), [(99, 0)])  # no haplotype is a column of the variants
    for bad in ([(1,)], [5], [(1, 2, 3)], [("a", 2)], [(1.5, 2)]):  # malformed windows
        with pytest.raises(ValueError):
            fm.site_frequency_spectrum(records(), two, windows=bad)
    with pytest.raises(ValueError):
        fm.site_frequency_spectrum(records(), two, windows=[(0, 10), (30, 20)])  # start > end
    with pytest.raises(ValueError):
        fm.site_frequency_spectrum(records(), two, region=(30, 20))
    pop = fm.Population("p", records(), two, 100)
    with pytest.raises(ValueError):
        pop.site_frequency_spectrum(windows=[(30, 20)])
    with pytest.raises(ValueError):
        pop.site_frequency_spectrum(windows=[(1,)])
    with pytest.raises(ValueError):
        fm.Population("q", records(), [], 100).site_frequency_spectrum()
    # nothing to count needs no device either: an empty variant list, a region or windows that hold no variant
    empty = fm.site_frequency_spectrum([], two)
    assert empty.sample_size == 2 and empty.counts.tolist() == [0, 0, 0]
    none = fm.site_frequency_spectrum(records(), two, region=(1000, 2000))
    assert none.sample_size == 2 and none.counts.tolist() == [0, 0, 0] and none.multiallelic_sites == 0 and none.incomplete_sites == 0
    none = fm.site_frequency_spectrum(records(), two, windows=[(1000, 2000), (-5, -1)])
    assert none.counts.shape == (2, 3) and not none.counts.any() and none.segregating_sites.tolist() == [0, 0]
    # two populations over different variant sets: hudson_fst's error
    other = fm.Population("o", records(n_sites=5), two, 100)
    with pytest.raises(ValueError) as err:
        fm.joint_site_frequency_spectrum(pop, other)
    with pytest.raises(ValueError) as err_fst:
        fm.hudson_fst(pop, other)
    assert str(err.value) == str(err_fst.value)
    # equal variants, but two resident matrices
    twin = fm.Population("t", records(), two, 100)
    with pytest.raises(ValueError) as err:
        fm.joint_site_frequency_spectrum(pop, twin)
    assert "ONE resident matrix" in str(err.value)
