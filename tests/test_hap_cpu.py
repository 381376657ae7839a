"""Haplotype homozygosity windows without a GPU: the exported symbols and their prototypes, the refusals that need no device and their
order, fmh_haplotype_stats against the plain-Python formulas of tests/hap_ref.py (every value is one division of two exactly converted
integers, so the comparison is == on the floats), and the Python surface (argument errors raised before any device use)."""

import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import hap_ref

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
    from ferromic_amd import _abi, device

    for name, n_args in (("fmh_haplotype_windows", 7), ("fmh_haplotype_stats", 4), ("fmh_haplotype_max_members", 0)):
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_abi.HapWindow) == 24 and C.sizeof(_abi.HapStatsOut) == 5 * 8
    assert device.HAP_WINDOW_DTYPE.itemsize == 24
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    for text in ("fmh_hap_window", "fmh_hap_stats_out", "fmh_haplotype_windows", "fmh_haplotype_stats", "fmh_haplotype_max_members", "FMH_HAP_THREADS"):
        assert text in header, text
    assert _abi.get_option("FMH_HAP_THREADS") == 0
    _abi.set_option("FMH_HAP_THREADS", 512)
    assert _abi.get_option("FMH_HAP_THREADS") == 512
    _abi.set_option("FMH_HAP_THREADS", None)
    assert _abi.get_option("FMH_HAP_THREADS") == 0


def test_the_cap_is_at_least_32768_and_stated_in_the_header(lib):
    from ferromic_amd import device

    cap = device.haplotype_max_members()
    assert cap >= 32768
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    assert f"{cap:,}".replace(",", " ") in header  # "34 304"
    # the cap is what the kernel's LDS layout holds in 160 KiB: a 512-byte head, 4 bytes of label per member, two bitmaps of 2 n bits and
    # one prefix per bitmap word (each rounded up to whole 16-byte vectors)
    def lds(n):
        words = ((n + 15) // 16 + 3) // 4 * 4
        return 512 + 4 * ((n + 3) // 4 * 4) + 3 * 4 * words

    assert lds(cap) <= 160 * 1024


def test_refusals_that_need_no_device_and_their_order(lib):
    from ferromic_amd import _abi

    out = np.zeros(3, dtype=np.uint64)
    windows = np.array([0, 0], dtype=np.uint64)
    o, w = out.ctypes.data_as(C.c_void_p), windows.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)  # never dereferenced: the NULL argument is found first
    for args, text in (((None, None, None, 0, None), b"NULL matrix"),      # every pointer NULL: the matrix is named
                       ((fake, None, None, 0, None), b"NULL groups"),      # then the groups
                       ((fake, fake, None, 0, None), b"h_windows"),        # then the windows
                       ((fake, fake, w, 0, None), b"d_out"),               # then the records (before n_windows == 0)
                       ((None, fake, w, 1, o), b"NULL matrix")):
        assert lib.fmh_haplotype_windows(args[0], args[1], args[2], args[3], args[4], None, None) == _abi.FMH_ERR_INVALID, text
        assert text in lib.fmh_last_error(), (text, lib.fmh_last_error())
    stats = np.zeros(5, dtype=np.float64)
    rec = np.zeros(1, dtype=[("sum_sq", np.uint64), ("distinct", np.uint32), ("top", np.uint32, (3,))])
    r, s = rec.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p)
    assert lib.fmh_haplotype_stats(None, 1, 4, s) == _abi.FMH_ERR_INVALID
    assert lib.fmh_haplotype_stats(r, 1, 4, None) == _abi.FMH_ERR_INVALID
    rec["sum_sq"], rec["distinct"], rec["top"] = 16, 1, [4, 0, 0]
    assert lib.fmh_haplotype_stats(r, 1, 0, s) == _abi.FMH_ERR_INVALID      # n = 0
    assert lib.fmh_haplotype_stats(r, 1, 4, s) == _abi.FMH_OK and stats[0] == 1.0
    assert lib.fmh_haplotype_stats(r, 1, 3, s) == _abi.FMH_ERR_INVALID      # sum_sq > n^2: not a partition of 3
    rec["sum_sq"] = 0
    assert lib.fmh_haplotype_stats(r, 1, 4, s) == _abi.FMH_ERR_INVALID
    assert lib.fmh_haplotype_stats(r, 0, 4, s) == _abi.FMH_OK               # no record, nothing to do


# ---- fmh_haplotype_stats ---------------------------------------------------------------------------------------------------------------
def check_stats(sizes):
    """Class sizes -> record -> fmh_haplotype_stats == the oracle's int / int, bit for bit."""
    from ferromic_amd import device

    sizes = sorted((int(c) for c in sizes), reverse=True)
    n = sum(sizes)
    sum_sq = sum(c * c for c in sizes)
    top = (sizes + [0, 0, 0])[:3]
    got = device.haplotype_stats([sum_sq], [len(sizes)], [top], n)
    ref = hap_ref.stats(sum_sq, top, n)
    for key in device.HAP_STATS:
        g, r = float(got[key][0]), ref[key]
        print(f"sizes={sizes[:6]} n={n} {key}: got {g!r} ref {r!r}")
        assert g == r or (math.isnan(g) and math.isnan(r)), (key, g, r)
    return {k: float(v[0]) for k, v in got.items()}


def test_stats_edge_partitions(lib):
    got = check_stats([1])  # n = 1
    assert got["h1"] == 1.0 and got["h12"] == 1.0 and got["h2_h1"] == 0.0 and math.isnan(got["haplotype_diversity"])
    got = check_stats([7])  # K = 1
    assert got["h1"] == 1.0 and got["h123"] == 1.0 and got["h2_h1"] == 0.0 and got["haplotype_diversity"] == 0.0
    got = check_stats([1] * 9)  # K = n
    assert got["h1"] == 1 / 9 and got["h12"] == 11 / 81 and got["h123"] == 15 / 81 and got["haplotype_diversity"] == 1.0
    got = check_stats([5, 3])  # K = 2: pooling the two classes gives one
    assert got["h12"] == 1.0 and got["h123"] == 1.0 and got["h1"] == 34 / 64 and got["h2_h1"] == 9 / 34
    got = check_stats([6, 4, 4, 1])  # a tie for second place
    assert got["h12"] == (69 + 48) / 225 and got["h123"] == (69 + 2 * (24 + 24 + 16)) / 225
    check_stats([3, 3, 3])  # a three-way tie
    check_stats([4, 4, 2, 2, 2])


def test_stats_random_partitions(lib):
    from ferromic_amd import device

    rng = np.random.default_rng(12)
    for n in (2, 3, 10, 257, 5000, device.haplotype_max_members()):
        for _ in range(4):
            cuts = np.sort(rng.choice(np.arange(1, n), size=min(n - 1, int(rng.integers(1, 40))), replace=False)) if n > 2 else np.array([1])
            sizes = np.diff(np.concatenate([[0], cuts, [n]]))
            check_stats(sizes)
    # several records in one call
    records = [([9, 1], 10), ([5, 5], 10), ([4, 3, 2, 1], 10)]
    got = device.haplotype_stats([sum(c * c for c in s) for s, _ in records], [len(s) for s, _ in records], [(s + [0, 0])[:3] for s, _ in records], 10)
    for w, (s, n) in enumerate(records):
        ref = hap_ref.stats(sum(c * c for c in s), (s + [0, 0])[:3], n)
        assert all(float(got[k][w]) == ref[k] for k in device.HAP_STATS)


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def records(n_sites=4, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


def test_python_surface_and_argument_errors(fm):
    """Every error here is raised before any device use: this test runs where there is no GPU."""
    assert callable(fm.garud_h) and callable(fm.Population.garud_h) and hasattr(fm.HaplotypeWindows, "first_identical")
    two = [(0, 0), (0, 1)]
    pop = fm.Population("p", records(), two, 100)
    for call in (lambda **kw: fm.garud_h(records(), two, **kw), lambda **kw: pop.garud_h(**kw)):
        with pytest.raises(ValueError, match="mutually exclusive"):
            call(windows=[(0, 10)], size=2)
        with pytest.raises(ValueError, match="mutually exclusive"):
            call(windows=[(0, 10)], step=2)
        with pytest.raises(ValueError, match="step needs size"):
            call(step=2)
        for bad in (0, -3, 1.5, "4"):
            with pytest.raises(ValueError, match="size must be a positive integer"):
                call(size=bad)
        with pytest.raises(ValueError, match="step must be a positive integer"):
            call(size=2, step=0)
        for bad in ([(1,)], [5], [(1, 2, 3)], [("a", 2)], [(1.5, 2)]):  # malformed windows, as the spectra
            with pytest.raises(ValueError):
                call(windows=bad)
        with pytest.raises(ValueError):
            call(windows=[(0, 10), (30, 20)])  # start > end
    with pytest.raises(ValueError):
        fm.garud_h(records(), [])  # too few haplotypes
    with pytest.raises(ValueError):
        fm.garud_h(records(), [(99, 0)])  # no haplotype is a column of the variants
    with pytest.raises(ValueError):
        fm.garud_h(records(), two, region=(30, 20))
    with pytest.raises(ValueError):
        fm.Population("q", records(), [], 100).garud_h()


def test_windows_without_a_row_need_no_device(fm):
    """An empty window is one class of everyone: no variant, a region or windows that hold no variant, size larger than the cohort."""
    three = [(0, 0), (0, 1), (2, 0)]
    for got in (fm.garud_h([], three), fm.garud_h(records(), three, region=(1000, 2000))):
        assert got.sample_size == 3 and len(got) == 1 and got.windows.tolist() == [[0, 0]]
        assert got.sum_squares.tolist() == [9] and got.distinct.tolist() == [1] and got.top_counts.tolist() == [[3, 0, 0]]
        assert got.h1.tolist() == [1.0] and got.h12.tolist() == [1.0] and got.h2_h1.tolist() == [0.0] and got.haplotype_diversity.tolist() == [0.0]
        assert got.first_identical is None
    got = fm.garud_h(records(), three, windows=[(1000, 2000), (-5, -1)], partition=True)
    assert len(got) == 2 and got.distinct.tolist() == [1, 1] and got.first_identical.tolist() == [[0, 0, 0], [0, 0, 0]]
    assert got.sum_squares.dtype == np.uint64 and got.distinct.dtype == np.uint32 and got.top_counts.dtype == np.uint32
    assert got.first_identical.dtype == np.uint32 and got.h123.dtype == np.float64 and got.windows.dtype == np.uint64
    assert "sample_size=3" in repr(got) and "windows=2" in repr(got)
    none = fm.garud_h(records(), three, size=5)  # four variants: no window of five fits
    assert len(none) == 0 and none.windows.shape == (0, 2) and none.h1.shape == (0,) and none.top_counts.shape == (0, 3)
    pop = fm.Population("p", records(), three, 100)
    assert pop.garud_h(windows=[(500, 600)]).distinct.tolist() == [1]
