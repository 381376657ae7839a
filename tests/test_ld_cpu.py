"""Linkage disequilibrium without a GPU: the host-only greedy rule (fmh_ld_prune_bits) against the plain-Python rule of tests/ld_ref.py,
the exported symbols and their prototypes, the Python surface and its argument checks, and the refusal to compute without a device.
Also the oracle against itself: its r^2 is the squared Pearson correlation of the indicator vectors over the jointly called columns."""

import ctypes as C
import os

import numpy as np
import pytest

from tests import ld_ref

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


def has_gpu():
    import torch

    return torch.cuda.is_available()


def random_over(rng, rows, band, density):
    words = (band + 31) // 32
    bits = rng.random((rows, words * 32)) < density
    # bits past the band are set on purpose: the rule must ignore them
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(rows, words).astype(np.uint32)


@pytest.mark.parametrize("rows", [0, 1, 33, 500])
@pytest.mark.parametrize("band", [1, 31, 32, 33, 100])
def test_prune_bits_matches_the_python_greedy(lib, rows, band):
    from ferromic_amd import device

    rng = np.random.default_rng(1000 * rows + band)
    for density in (0.02, 0.3, 0.9):
        over = random_over(rng, rows, band, density)
        got = device.ld_prune_bits(over, band)
        assert got.dtype == bool and got.shape == (rows,)
        assert np.array_equal(got, ld_ref.greedy_from_bits(over, band)), (rows, band, density)


def test_prune_bits_removal_is_not_transitive(lib):
    """r2(0,1) and r2(1,2) high, r2(0,2) low: site 1 goes, and being removed it removes nothing - site 2 stays."""
    from ferromic_amd import device

    over = np.array([[0b01], [0b01], [0b00]], dtype=np.uint32)  # row 0: d = 1 set, d = 2 clear; row 1: d = 1 set
    assert device.ld_prune_bits(over, 2).tolist() == [True, False, True]
    assert ld_ref.greedy_from_bits(over, 2).tolist() == [True, False, True]
    r2 = np.array([[0.9, 0.1], [0.9, np.nan], [np.nan, np.nan]])
    assert ld_ref.greedy_from_r2(r2, 0.5).tolist() == [True, False, True]


def test_prune_bits_refuses_bad_arguments(lib):
    from ferromic_amd import _abi

    keep = np.zeros(4, dtype=np.uint8)
    over = np.zeros((4, 1), dtype=np.uint32)
    assert lib.fmh_ld_prune_bits(over.ctypes.data_as(C.c_void_p), 4, 0, keep.ctypes.data_as(C.c_void_p)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_ld_prune_bits(None, 4, 3, keep.ctypes.data_as(C.c_void_p)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_ld_prune_bits(None, 0, 3, None) == _abi.FMH_OK


def test_symbols_are_exported_and_prototyped(lib):
    from ferromic_amd import _abi

    for name, n_args in (("fmh_ld_band", 11), ("fmh_ld_prune", 8), ("fmh_ld_prune_bits", 4), ("fmh_ld_prune_chunked", 9)):
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_abi.LdBandOut) == 4 * C.sizeof(C.c_void_p)
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    assert "#define FMH_ABI_VERSION 3" in header and "fmh_ld_band_out" in header


def test_python_surface(fm):
    assert callable(fm.ld_r2) and callable(fm.ld_prune)
    assert callable(fm.Population.ld_r2) and callable(fm.Population.ld_prune)


def records(n_sites=4, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


def test_value_errors(fm):
    two = [(0, 0), (0, 1)]
    with pytest.raises(ValueError):
        fm.ld_r2(records(), [(0, 0)], 3)  # fewer than two haplotypes
    with pytest.raises(ValueError):
        fm.ld_prune(records(), [], 3, 0.2)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            fm.ld_r2(records(), two, bad)
        with pytest.raises(ValueError):
            fm.ld_prune(records(), two, bad, 0.2)
    for bad in (float("nan"), -0.01, 1.01, float("inf")):
        with pytest.raises(ValueError):
            fm.ld_prune(records(), two, 3, bad)
    pop = fm.Population("p", records(), two, 100)
    one = fm.Population("q", records(), [(1, 0)], 100)
    with pytest.raises(ValueError):
        one.ld_r2(3)
    with pytest.raises(ValueError):
        one.ld_prune(3, 0.2)
    with pytest.raises(ValueError):
        pop.ld_r2(0)
    with pytest.raises(ValueError):
        pop.ld_prune(0, 0.2)
    with pytest.raises(ValueError):
        pop.ld_prune(3, float("nan"))
    with pytest.raises(ValueError):
        pop.ld_prune(3, 1.5)


def test_empty_inputs_give_empty_arrays(fm):
    two = [(0, 0), (0, 1)]
    r2 = fm.ld_r2([], two, 5)
    assert isinstance(r2, np.ndarray) and r2.dtype == np.float64 and r2.shape == (0, 5)
    keep = fm.ld_prune([], two, 5, 0.2)
    assert isinstance(keep, np.ndarray) and keep.dtype == bool and keep.shape == (0,)
    # a region that holds no variant
    assert fm.ld_r2(records(), two, 5, region=(1000, 2000)).shape == (0, 5)
    assert fm.ld_prune(records(), two, 5, 0.2, region=(1000, 2000)).shape == (0,)


def test_no_gpu_no_result(lib, fm):
    """Without a device every call that would count fails loudly: there is no CPU route behind the API."""
    if has_gpu():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    from ferromic_amd import _abi

    two = [(0, 0), (0, 1)]
    with pytest.raises(RuntimeError):
        fm.ld_r2(records(), two, 2)
    with pytest.raises(RuntimeError):
        fm.ld_prune(records(), two, 2, 0.2)
    pop = fm.Population("p", records(), two, 100)
    with pytest.raises(RuntimeError):
        pop.ld_r2(2)
    with pytest.raises(RuntimeError):
        pop.ld_prune(2, 0.2)
    dense = fm.Population.from_numpy("d", np.zeros((4, 3, 2), dtype=np.int8), np.arange(4, dtype=np.int64), two, 100)
    with pytest.raises(RuntimeError):
        dense.ld_r2(2)
    # at the C-ABI no matrix can exist without a device; the calls refuse a NULL one instead of computing
    out = _abi.LdBandOut()
    keep = np.zeros(4, dtype=np.uint8)
    assert lib.fmh_ld_band(None, None, 0, 4, 4, 2, 0.5, C.byref(out), None, None, None) != _abi.FMH_OK
    assert lib.fmh_ld_prune(None, None, 0, 4, 2, 0.5, keep.ctypes.data_as(C.c_void_p), None) != _abi.FMH_OK
    with pytest.raises(_abi.NoDeviceError):
        _abi.device_count()


def test_oracle_is_the_squared_correlation():
    """200 x 130 with gaps, allele 2 and a column mask: the oracle's r^2 equals corrcoef^2 over the jointly called, member columns."""
    rng = np.random.default_rng(7)
    S, H, B = 200, 130, 9
    x = (rng.random((S, H)) < rng.uniform(0.1, 0.9, size=(S, 1))).astype(np.uint8)
    x[rng.random((S, H)) < 0.05] = 2
    called = rng.random((S, H)) >= 0.03
    mask = rng.random(H) < 0.7
    ref = ld_ref.band(x, called, mask, 0, S, S, B, 0.0)
    worst = 0.0
    for i in range(S):
        for d in range(1, B + 1):
            j = i + d
            if j >= S:
                assert np.isnan(ref["r2"][i, d - 1])
                continue
            cols = called[i] & called[j] & mask
            a, b = (x[i, cols] >= 1).astype(float), (x[j, cols] >= 1).astype(float)
            assert ref["n_joint"][i, d - 1] == cols.sum()
            if a.std() == 0 or b.std() == 0:
                assert np.isnan(ref["r2"][i, d - 1])
                continue
            worst = max(worst, abs(ref["r2"][i, d - 1] - np.corrcoef(a, b)[0, 1] ** 2))
    assert worst <= 1e-13, worst
