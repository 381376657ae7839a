"""Extended haplotype homozygosity scans without a GPU: the oracle of tests/ehh_ref.py against a second, brute-force definition and a case
worked by hand; fmh_ehh_stats against the oracle (== on the quotients, at most 2 ulp on the two logarithms: libm's log need not be correctly
rounded, the quotient inside it is the same double on both sides); the refusals of fmh_ehh_scan that are found before a handle is read, and
their order (those that read a handle are in tests/test_gpu_ehh.py); every ValueError of the Python surface, raised before any device use;
fmh_ehh_max_members; the exported names."""

import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import ehh_ref

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


# ---- the oracle itself -------------------------------------------------------------------------------------------------------------------
def test_oracle_pair_steps_equal_the_brute_force_sum_over_pairs():
    """Without a threshold and a gap rule pair_steps is, per core, the sum over its pairs of the flank the two members share."""
    rows, cols = 120, 48
    x = ehh_ref.mosaic(rows, cols, founders=4, switch=0.02, mutation=0.004, seed=5).copy()
    rng = np.random.default_rng(6)
    x[rng.random(x.shape) < 0.01] = 2
    called = rng.random(x.shape) > 0.02
    mask = rng.random(cols) < 0.8
    checked = 0
    for row_begin, row_end, max_extent in ((0, rows, 0), (17, 101, 0), (0, rows, 9)):
        focal = [row_begin, row_begin + 3, (row_begin + row_end) // 2, row_end - 2, row_end - 1]
        sides, _ = ehh_ref.scan(x, called, mask, focal, row_begin, row_end, max_extent=max_extent)
        for i, f in enumerate(focal):
            for s, side in enumerate((-1, 1)):
                brute = ehh_ref.brute_pair_steps(x, called, mask, f, side, row_begin, row_end, max_extent)
                assert sides[i, s]["pair_steps"].tolist() == brute, (row_begin, row_end, max_extent, f, side)
                checked += sum(brute)
                # unit distance: the area is the trapezoid sum of the same curve, which ended at P = 0 unless the core met the edge
                p_init = [int(c) * (int(c) - 1) // 2 for c in sides[i, s]["core"]]
                for a in (0, 1):
                    if sides[i, s]["steps"][a] and not sides[i, s]["flags"] & (ehh_ref.EDGE0 << a):
                        assert int(sides[i, s]["area2"][a]) == p_init[a] + 2 * brute[a]
    assert checked > 1000


def hand_made():
    """3 rows x 8 columns, focal row 0: five carriers whose next rows read [0,0,1,2,3] and [0,1,1,2,3], three non-carriers that stay identical."""
    x = np.zeros((3, 8), dtype=np.uint8)
    x[0, :5] = 1
    x[1, :5] = [0, 0, 1, 2, 3]
    x[2, :5] = [0, 1, 1, 2, 3]
    return x, np.array([10, 10, 4_000_000_000], dtype=np.uint32)


def test_oracle_on_the_case_worked_by_hand():
    x, positions = hand_made()
    mask = np.ones(8, dtype=bool)
    sides, pairs = ehh_ref.scan(x, None, mask, [0], positions=positions, min_ehh=(1, 10), max_extent=2, curve=True)
    left, right = sides[0]
    assert left["core"].tolist() == [3, 5] and left["steps"].tolist() == [0, 0] and left["flags"] == ehh_ref.EDGE0 | ehh_ref.EDGE1
    # core 1: P(0) = 10, P(1) = 1 and 1 * 10 == 10 * 1, so the step counts (gap 0: no area); P(2) = 0 is below the threshold: not counted
    assert right["steps"].tolist() == [2, 1] and right["pair_steps"].tolist() == [6, 1]
    # core 0: P = 3 throughout; (3 + 3) * 0 + (3 + 3) * 3 999 999 990, and still alive at the end of the range
    assert right["area2"].tolist() == [23_999_999_940, 0] and right["flags"] == ehh_ref.EDGE0
    assert pairs[0, 1].tolist() == [[3, 3], [1, 0]] and not pairs[0, 0].any()
    # one hundredth above the threshold the first step stops
    sides, _ = ehh_ref.scan(x, None, mask, [0], positions=positions, min_ehh=(11, 100), max_extent=2)
    assert sides[0, 1]["steps"].tolist() == [2, 0] and sides[0, 1]["pair_steps"].tolist() == [6, 0]


# ---- symbols ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_prototyped(lib, fm):
    from ferromic_amd import _abi, device

    for name, n_args in (("fmh_ehh_scan", 11), ("fmh_ehh_stats", 4), ("fmh_ehh_max_members", 0)):
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_abi.EhhSide) == 56 and C.sizeof(_abi.EhhParams) == 24 and C.sizeof(_abi.EhhStatsOut) == 6 * 8
    assert device.EHH_SIDE_DTYPE.itemsize == 56 and ehh_ref.SIDE_DTYPE == device.EHH_SIDE_DTYPE
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    for text in ("fmh_ehh_side", "fmh_ehh_params", "fmh_ehh_stats_out", "fmh_ehh_scan", "fmh_ehh_stats", "fmh_ehh_max_members", "FMH_EHH_SKIPPED"):
        assert text in header, text
    assert (device.EHH_EDGE0, device.EHH_EDGE1, device.EHH_GAP0, device.EHH_GAP1, device.EHH_SKIPPED) == (1, 2, 4, 8, 16)
    for name in ("ehh_scan", "ihs", "nsl", "HaplotypeScan"):
        assert hasattr(fm, name), name
    for name in ("ehh_scan", "ihs", "nsl"):
        assert callable(getattr(fm.Population, name)), name
    for name in ("sample_size", "focal_rows", "core_counts", "area2", "pair_steps", "steps", "flags", "ihh", "sl", "ihs", "nsl", "pairs"):
        assert hasattr(fm.HaplotypeScan, name), name


def test_the_cap_is_that_of_the_haplotype_windows_and_stated_in_the_header(lib):
    from ferromic_amd import device

    cap = device.ehh_max_members()
    assert cap == device.haplotype_max_members() and cap >= 32768
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    section = header[header.index("fmh_ehh_max_members (needs no device)"):]
    assert f"{cap:,}".replace(",", " ") in section[:400]


def test_refusals_that_need_no_device_and_their_order(lib):
    from ferromic_amd import _abi

    out = np.zeros(14, dtype=np.uint64)
    focal = np.zeros(1, dtype=np.uint64)
    params = _abi.EhhParams(0, 1, 0, 0, 0, 0)
    o, f, p = out.ctypes.data_as(C.c_void_p), focal.ctypes.data_as(C.c_void_p), C.byref(params)
    fake = C.c_void_p(16)  # never dereferenced: the NULL argument is found first
    for args, text in (((None, None, None, None, None), b"NULL matrix"),
                       ((fake, None, None, None, None), b"NULL groups"),
                       ((fake, fake, None, None, None), b"h_focal"),
                       ((fake, fake, f, None, None), b"params"),
                       ((fake, fake, f, p, None), b"d_out"),
                       ((None, fake, f, p, o), b"NULL matrix")):
        m, g, focal_ptr, params_ptr, d_out = args
        assert lib.fmh_ehh_scan(m, g, 0, 1, focal_ptr, 1, None, params_ptr, d_out, None, None) == _abi.FMH_ERR_INVALID, text
        assert text in lib.fmh_last_error(), (text, lib.fmh_last_error())
    stats = np.zeros(6, dtype=np.float64)
    sides = np.zeros(2, dtype=ehh_ref.SIDE_DTYPE)
    s, r = stats.ctypes.data_as(C.c_void_p), sides.ctypes.data_as(C.c_void_p)
    assert lib.fmh_ehh_stats(None, 1, 0, s) == _abi.FMH_ERR_INVALID
    assert lib.fmh_ehh_stats(r, 1, 0, None) == _abi.FMH_ERR_INVALID
    assert lib.fmh_ehh_stats(r, 0, 0, s) == _abi.FMH_OK  # no record, nothing to do
    assert lib.fmh_ehh_stats(r, 1, 0, s) == _abi.FMH_OK and np.isnan(stats).all()  # both cores empty
    sides["core"] = [[4, 4], [4, 5]]
    assert lib.fmh_ehh_stats(r, 1, 0, s) == _abi.FMH_ERR_INVALID  # the two sides are not of one focal row
    sides["core"] = [[4, 4], [4, 4]]
    sides["flags"] = [0, ehh_ref.SKIPPED]
    assert lib.fmh_ehh_stats(r, 1, 0, s) == _abi.FMH_ERR_INVALID


# ---- fmh_ehh_stats ---------------------------------------------------------------------------------------------------------------------
def ulps_apart(a, b):
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))


def assert_stats_equal(got, ref, what=""):
    for key in ("ihh", "sl"):
        assert got[key].shape == ref[key].shape
        assert np.array_equal(got[key], ref[key], equal_nan=True), (what, key)
    for key in ("ihs", "nsl"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), (what, key)
        worst = max([ulps_apart(g, r) for g, r in zip(got[key], ref[key]) if not math.isnan(r)], default=0)
        print(f"{what} {key}: worst distance {worst} ulp over {int((~np.isnan(ref[key])).sum())} values")
        assert worst <= 2, (what, key, worst)


def test_stats_against_the_oracle(lib):
    from ferromic_amd import device

    rows, cols = 300, 40
    x = ehh_ref.mosaic(rows, cols, founders=5, switch=0.05, mutation=0.01, seed=8)
    positions = np.cumsum(np.random.default_rng(9).integers(0, 1000, size=rows)).astype(np.uint32)
    mask = np.ones(cols, dtype=bool)
    sides, _ = ehh_ref.scan(x, None, mask, range(rows), positions=positions, min_ehh=(1, 20), max_gap=980, min_core=3)
    flags = sides["flags"]
    assert (flags & ehh_ref.SKIPPED).any() and (flags & (ehh_ref.GAP0 | ehh_ref.GAP1)).any() and (flags & (ehh_ref.EDGE0 | ehh_ref.EDGE1)).any()
    for include_edges in (False, True):
        ref = ehh_ref.stats(sides, include_edges)
        assert_stats_equal(device.ehh_stats(sides, include_edges), ref, f"include_edges={include_edges}")
        assert np.isfinite(ref["ihs"]).sum() > (40 if include_edges else 10) and np.isnan(ref["ihs"]).any()
    assert np.isfinite(ehh_ref.stats(sides, True)["ihs"]).sum() > np.isfinite(ehh_ref.stats(sides, False)["ihs"]).sum()


def test_stats_edge_records(lib):
    from ferromic_amd import device

    sides = np.zeros((6, 2), dtype=ehh_ref.SIDE_DTYPE)
    sides["core"] = [7, 5]
    sides["area2"][:, 0], sides["area2"][:, 1] = [30, 11], [2**62 + 12345, 2**62 + 1]  # sums beyond 2^53: one rounding in the conversion
    sides["pair_steps"][:, 0], sides["pair_steps"][:, 1] = [40, 9], [3, 8]
    sides["core"][1] = [7, 1]                      # a singleton core: P_1(0) = 0
    sides["flags"][2] = ehh_ref.SKIPPED
    sides["flags"][3, 1] = ehh_ref.EDGE1           # one flag on one side
    sides["flags"][4, 0] = ehh_ref.GAP0
    sides["area2"][5] = 0                          # an operand of the quotient is 0
    for include_edges in (False, True):
        got, ref = device.ehh_stats(sides, include_edges), ehh_ref.stats(sides, include_edges)
        assert_stats_equal(got, ref, "edge records")
        assert np.isfinite(got["ihs"][0]) and got["ihh"][0, 0] == float(2**62 + 12375) / float(42)
        assert np.isnan(got["ihs"][1]) and np.isnan(got["ihh"][1, 1]) and np.isfinite(got["ihh"][1, 0])
        assert np.isnan(got["ihh"][2]).all() and np.isnan(got["nsl"][2])
        assert np.isfinite(got["ihs"][3]) == include_edges and np.isfinite(got["nsl"][4]) == include_edges
        assert got["ihh"][5].tolist() == [0.0, 0.0] and np.isnan(got["ihs"][5]) and np.isfinite(got["nsl"][5])


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def records(n_sites=6, n_samples=3, positions=None):
    positions = [10 * i for i in range(n_sites)] if positions is None else positions
    return [dict(position=positions[i], genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


def test_python_argument_errors(fm):
    """Every error here is raised before any device use: this test runs where there is no GPU."""
    four = [(0, 0), (0, 1), (1, 0), (2, 1)]
    pop = fm.Population("p", records(), four, 100)
    for call in (lambda **kw: fm.ehh_scan(records(), four, **kw), lambda **kw: pop.ehh_scan(**kw)):
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="min_ehh"):
                call(min_ehh=bad)
            with pytest.raises(ValueError, match="min_maf"):
                call(min_maf=bad)
        for bad in (0, -3, 1.5, "4", 2**32):
            with pytest.raises(ValueError, match="max_extent"):
                call(max_extent=bad)
            with pytest.raises(ValueError, match="max_gap"):
                call(max_gap=bad)
        with pytest.raises(ValueError, match="curve=True needs a max_extent"):
            call(curve=True)
        for bad in ([1.5], ["a"], [-1]):
            with pytest.raises(ValueError, match="focal"):
                call(focal=bad)
        with pytest.raises(ValueError, match="focal row 6 is outside the 6 variants"):
            call(focal=[0, 6])
    for call in (lambda **kw: fm.ihs(records(), four, **kw), lambda **kw: pop.ihs(**kw), lambda **kw: fm.nsl(records(), four, **kw), lambda **kw: pop.nsl(**kw)):
        with pytest.raises(ValueError, match="max_extent"):
            call(max_extent=0)
        with pytest.raises(ValueError, match="focal row"):
            call(focal=[99])
    # positions: below 0, above 2^32 - 1, descending - not looked at under unit distance until a device is needed
    for positions, text in (([-5, 0, 10, 20, 30, 40], "outside 0"), ([0, 10, 20, 30, 40, 2**32], "outside 0"), ([0, 10, 20, 15, 30, 40], "descend")):
        with pytest.raises(ValueError, match=text):
            fm.ehh_scan(records(positions=positions), four)
        with pytest.raises(ValueError, match=text):
            fm.ihs(records(positions=positions), four)
        with pytest.raises(ValueError, match=text):
            fm.Population("q", records(positions=positions), four, 2**33).ihs()
    with pytest.raises(ValueError):
        fm.ehh_scan(records(), [])  # too few haplotypes
    with pytest.raises(ValueError):
        fm.ihs(records(), [(99, 0)])  # no haplotype is a column of the variants
    with pytest.raises(ValueError):
        fm.nsl(records(), four, region=(30, 20))
    with pytest.raises(ValueError):
        fm.Population("q", records(), [], 100).nsl()


def test_scans_without_a_focal_row_need_no_device(fm):
    three = [(0, 0), (0, 1), (2, 0)]
    for got in (fm.ehh_scan([], three), fm.ihs(records(), three, region=(1000, 2000)), fm.nsl(records(), three, focal=[]),
                fm.ehh_scan(records(), three, focal=[], max_extent=4, curve=True), fm.Population("p", records(), three, 100).ehh_scan(focal=[])):
        assert got.sample_size == 3 and len(got) == 0 and got.focal_rows.shape == (0,) and got.focal_rows.dtype == np.uint64
        assert got.core_counts.shape == (0, 2) and got.core_counts.dtype == np.uint32
        assert got.area2.shape == (0, 2, 2) and got.area2.dtype == np.uint64 and got.pair_steps.shape == (0, 2, 2) and got.pair_steps.dtype == np.uint64
        assert got.steps.shape == (0, 2, 2) and got.steps.dtype == np.uint32 and got.flags.shape == (0, 2) and got.flags.dtype == np.uint32
        assert got.ihh.shape == (0, 2) and got.sl.shape == (0, 2) and got.ihs.shape == (0,) and got.nsl.shape == (0,) and got.ihs.dtype == np.float64
        assert "sample_size=3" in repr(got) and "focal=0" in repr(got)
    assert fm.ehh_scan(records(), three, focal=[], max_extent=4, curve=True).pairs.shape == (0, 2, 2, 4)
    assert fm.nsl(records(), three, focal=[]).pairs is None
    with pytest.raises(ValueError, match="focal row 0 is outside the 0 variants"):
        fm.ehh_scan([], three, focal=[0])
