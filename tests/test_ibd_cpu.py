"""IBD segments without a GPU: the host twin (fmh_ibd_scan_host) and fmh_ibd_sort_segments against tests/ibd_ref.py, the oracle written
from the definition - every table with array_equal, the segments as sorted lists.

Hand-worked cases first: each pins one rule of the definition with the expected runs written out by hand (not computed), and both the
oracle and the twin have to give them.  Then the twin against the oracle on planted cohorts over n x K x mode, bare and with a keep mask,
positions and every filter.  Last, the twin compiled into a stand-alone program under AddressSanitizer + UBSan on a cohort this file
restates from the same integer stream."""

import os
import subprocess

import numpy as np
import pytest

from tests import ibd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.path.join(ROOT, "ferromic_amd", "bin")
LOOSE = dict(min_sites=1, min_length=1, max_gap=0, max_bp_per_site=0)
FULL = dict(min_sites=12, min_length=9_000, max_gap=1_000_000, max_bp_per_site=1_250, max_missing=2)


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import device

    return device


def device_params(dev, p):
    return dev.ibd_params(mode=p["mode"], min_sites=p["min_sites"], min_length=p["min_length"], max_gap=p["max_gap"],
                          max_bp_per_site=p["max_bp_per_site"], max_missing=None if p["max_missing"] == R.NO_LIMIT else p["max_missing"])


def assert_same(got, ref, what):
    """An IbdResult of the library against the oracle's dict."""
    for name in R.TABLES:
        assert got.tables[name].dtype == np.uint64 and got.tables[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(got.tables[name], ref[name]), (what, name, got.tables[name], ref[name])
    assert got.count == len(ref["segments"]), what
    assert R.segment_tuples(got.segments) == ref["segments"], what


def both(dev, columns, x=None, **kw):
    """Oracle and twin over one dosage string per sample ('0', '1', '2'; '3' = not called); the twin has to equal the oracle; returns the
    oracle's result with the runs as (a, b, first, last, n_missing) for the literal comparison."""
    dosage = np.array([[int(c) for c in col] for col in columns], dtype=np.uint8).T.reshape(len(columns[0]), len(columns))
    p = R.params(**{**LOOSE, **kw})
    ref = R.scan(dosage, x, p)
    got = dev.ibd_scan_host(dosage, device_params(dev, p), x=x, capacity=64)
    assert_same(got, ref, (columns, kw))
    ref["spans"] = [(s[0], s[1], s[4], s[5], s[3]) for s in ref["segments"]]
    return ref


def test_symbols_are_exported_and_prototyped(dev):
    from ferromic_amd import _abi

    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    for name, n_args in (("fmh_ibd_scan", 13), ("fmh_ibd_scan_host", 9), ("fmh_ibd_sort_segments", 2)):
        assert hasattr(lib, name) and name in _abi.SYMBOLS and ("int " + name + "(") in header and len(_abi.SYMBOLS[name][1]) == n_args, name
    assert _abi.get_option("FMH_IBD_ITEM_ROWS") == 0 and _abi.get_option("FMH_IBD_BUDGET_BYTES") == 4 << 30
    import ctypes as C

    assert C.sizeof(_abi.IbdParams) == 24 and C.sizeof(_abi.IbdSegment) == 32 == dev.IBD_SEGMENT_DTYPE.itemsize and C.sizeof(_abi.IbdOut) == 32
    assert "#define FMH_IBD1 1" in header and "#define FMH_IBD2 2" in header and (dev.IBD1, dev.IBD2) == (1, 2)


# ---- hand-worked cases: the expected values are written out, not computed -----------------------------------------------------------------
def test_one_kept_row(dev):
    assert both(dev, ["0", "0"])["spans"] == [(0, 1, 0, 0, 0)]
    assert both(dev, ["0", "2"])["spans"] == []                                     # opposite homozygotes
    assert both(dev, ["0", "3"])["spans"] == [(0, 1, 0, 0, 1)]                      # a MISS row is compatible
    assert both(dev, ["0", "1"], mode=R.IBD2)["spans"] == []
    one = both(dev, ["0", "0"])
    assert one["n_segments"].tolist() == [[0, 1], [1, 0]] and one["sum_length"].tolist() == [[0, 1], [1, 0]]


def test_disc_at_the_first_and_at_the_last_row(dev):
    assert both(dev, ["00000", "20000"])["spans"] == [(0, 1, 1, 4, 0)]
    assert both(dev, ["00000", "00002"])["spans"] == [(0, 1, 0, 3, 0)]
    assert both(dev, ["00000", "20002"])["spans"] == [(0, 1, 1, 3, 0)]


def test_every_row_disc_and_no_row_disc(dev):
    none = both(dev, ["0000", "2222"])
    assert none["spans"] == [] and not none["n_segments"].any() and not none["longest_length"].any()
    whole = both(dev, ["0120", "0120"], mode=R.IBD2)
    assert whole["spans"] == [(0, 1, 0, 3, 0)] and whole["sum_sites"].tolist() == [[0, 4], [4, 0]]


def test_a_single_disc_row_ends_a_run(dev):
    ref = both(dev, ["0000000", "0002000"])
    assert ref["spans"] == [(0, 1, 0, 2, 0), (0, 1, 4, 6, 0)]
    assert ref["n_segments"][0, 1] == 2 and ref["sum_sites"][1, 0] == 6 and ref["longest_length"][0, 1] == 3


def test_a_miss_row_stands_at_a_runs_end_and_is_not_trimmed(dev):
    ref = both(dev, ["2003002", "0003330"])                                         # rows 0 and 6 DISC; rows 3, 4, 5 MISS
    assert ref["spans"] == [(0, 1, 1, 5, 3)]
    ref = both(dev, ["3002", "0000"])                                               # the run starts on a MISS row
    assert ref["spans"] == [(0, 1, 0, 2, 1)]
    ref = both(dev, ["2003", "0000"])                                               # ... and ends on one
    assert ref["spans"] == [(0, 1, 1, 3, 1)]


def test_a_het_against_a_hom_in_each_mode(dev):
    cols = ["0001000", "0000000"]                                                   # row 3: het against hom-ref
    assert both(dev, cols, mode=R.IBD1)["spans"] == [(0, 1, 0, 6, 0)]
    assert both(dev, cols, mode=R.IBD2)["spans"] == [(0, 1, 0, 2, 0), (0, 1, 4, 6, 0)]
    cols = ["0001000", "0002000"]                                                   # het against hom-alt
    assert both(dev, cols, mode=R.IBD1)["spans"] == [(0, 1, 0, 6, 0)]
    assert both(dev, cols, mode=R.IBD2)["spans"] == [(0, 1, 0, 2, 0), (0, 1, 4, 6, 0)]
    cols = ["1111", "1111"]                                                         # het against het: concordant in both
    assert both(dev, cols, mode=R.IBD1)["spans"] == both(dev, cols, mode=R.IBD2)["spans"] == [(0, 1, 0, 3, 0)]


def test_gap_exactly_max_gap_and_one_more(dev):
    cols = ["000000", "000000"]
    x = np.array([0, 10, 20, 120, 130, 140])
    assert both(dev, cols, x=x, max_gap=100)["spans"] == [(0, 1, 0, 5, 0)]          # the gap of 100 is not above max_gap
    assert both(dev, cols, x=x, max_gap=99)["spans"] == [(0, 1, 0, 2, 0), (0, 1, 3, 5, 0)]
    assert both(dev, cols, x=x, max_gap=0)["spans"] == [(0, 1, 0, 5, 0)]            # 0 = no limit
    cut = both(dev, cols, x=x, max_gap=99)
    assert cut["sum_length"][0, 1] == 21 + 21 and cut["longest_length"][0, 1] == 21


def test_every_filter_exactly_met_and_missed_by_one(dev):
    cols = ["0000030000", "0000000000"]                                             # one run of 10 sites, 1 missing
    x = np.arange(10) * 10                                                          # length 91
    met = dict(min_sites=10, min_length=91, max_missing=1, max_bp_per_site=10)     # 91 <= 10 * 10
    assert both(dev, cols, x=x, **met)["spans"] == [(0, 1, 0, 9, 1)]
    for missed in (dict(min_sites=11), dict(min_length=92), dict(max_missing=0), dict(max_bp_per_site=9)):   # 91 > 9 * 10
        assert both(dev, cols, x=x, **{**met, **missed})["spans"] == [], missed
    assert both(dev, cols, x=x, **{**met, "max_bp_per_site": 0})["spans"] == [(0, 1, 0, 9, 1)]


def test_three_samples_keep_their_pairs(dev):
    ref = both(dev, ["00000", "00200", "22222"])
    assert ref["spans"] == [(0, 1, 0, 1, 0), (0, 1, 3, 4, 0), (1, 2, 2, 2, 0)]
    assert ref["n_segments"].tolist() == [[0, 2, 0], [2, 0, 1], [0, 1, 0]]
    assert np.array_equal(ref["sum_sites"], ref["sum_sites"].T) and not np.diag(ref["sum_sites"]).any()


def test_no_row_and_one_sample(dev):
    p = dev.ibd_params(**LOOSE)
    none = dev.ibd_scan_host(np.zeros((0, 3), dtype=np.uint8), p, capacity=4)
    assert none.count == 0 and all(t.shape == (3, 3) and not t.any() for t in none.tables.values())
    one = dev.ibd_scan_host(np.zeros((5, 1), dtype=np.uint8), p, capacity=4)
    assert one.count == 0 and all(t.shape == (1, 1) and not t.any() for t in one.tables.values())


def test_scan_refusals(dev):
    from ferromic_amd import _abi

    dosage = np.zeros((4, 2), dtype=np.uint8)
    ok = dev.ibd_params(**LOOSE)
    for mode in (0, 3):
        with pytest.raises(_abi.FerromicHipError, match="mode"):
            dev.ibd_scan_host(dosage, dev.ibd_params(mode=mode, **LOOSE), capacity=4)
    with pytest.raises(_abi.FerromicHipError, match="descend"):
        dev.ibd_scan_host(dosage, ok, x=np.array([0, 5, 4, 9]), capacity=4)
    with pytest.raises(_abi.FerromicHipError, match="dosage 4"):
        dev.ibd_scan_host(np.full((4, 2), 4, dtype=np.uint8), ok, capacity=4)
    lib = _abi.load()
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, None, 4, 2, None, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"params" in lib.fmh_last_error()
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, None, 4, 0, ok, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"n_samples" in lib.fmh_last_error()
    assert lib.fmh_ibd_scan_host(None, None, 4, 2, ok, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"dosage" in lib.fmh_last_error()
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, None, 4, 2, ok, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"every output" in lib.fmh_last_error()
    seg = np.zeros(4, dtype=dev.IBD_SEGMENT_DTYPE)
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, None, 4, 2, ok, None, seg.ctypes.data, 4, None) == _abi.FMH_ERR_INVALID
    assert b"h_segment_count" in lib.fmh_last_error()
    # the mode is refused before the positions, the positions before the outputs
    bad_mode = dev.ibd_params(mode=7, **LOOSE)
    down = np.array([3, 2, 1, 0], dtype=np.uint32)
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, down.ctypes.data, 4, 2, bad_mode, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"mode" in lib.fmh_last_error()
    assert lib.fmh_ibd_scan_host(dosage.ctypes.data, down.ctypes.data, 4, 2, ok, None, None, 0, None) == _abi.FMH_ERR_INVALID and b"descend" in lib.fmh_last_error()
    # the device entry point's refusals that need no handle
    assert lib.fmh_ibd_scan(None, None, 2, 0, 4, None, None, ok, None, None, 0, None, None) == _abi.FMH_ERR_INVALID and b"NULL matrix" in lib.fmh_last_error()
    # capacity below the count: the count stays exact, the buffer holds that many true segments
    d = np.zeros((12, 3), dtype=np.uint8)
    d[5, 0] = 2
    ref = R.scan(d, None, R.params(**LOOSE))
    few = dev.ibd_scan_host(d, ok, capacity=2)
    assert few.count == 5 == len(ref["segments"]) and len(few.segments) == 2 and set(R.segment_tuples(few.segments)) <= set(ref["segments"])
    none = dev.ibd_scan_host(d, ok, capacity=0)
    assert none.count == 5 and len(none.segments) == 0
    counted = dev.ibd_scan_host(d, ok)
    assert counted.count is None and np.array_equal(counted.tables["n_segments"], ref["n_segments"])


def test_sort_segments(dev):
    rng = np.random.default_rng(5)
    seg = np.zeros(300, dtype=dev.IBD_SEGMENT_DTYPE)
    seg["a"] = rng.integers(0, 5, size=300)
    seg["b"] = seg["a"] + 1 + rng.integers(0, 4, size=300)
    seg["first_row"] = rng.permutation(300) * 3
    seg["last_row"] = seg["first_row"] + 2
    seg["n_sites"] = np.arange(300)
    got = dev.ibd_sort_segments(seg)
    order = np.lexsort((seg["first_row"], seg["b"], seg["a"]))
    assert np.array_equal(got, seg[order]) and len(dev.ibd_sort_segments(seg[:0])) == 0


# ---- the twin against the oracle on planted cohorts ------------------------------------------------------------------------------------------
NS, KS = (1, 2, 3, 33), (0, 1, 2, 63, 64, 65, 200, 400)


def test_planted_cohorts_meet_the_preconditions():
    """On the oracle alone: the planted cohorts hold IBD1 and IBD2 runs of 15..70 rows, pairs with different counts, one run over everything,
    and the uniform background holds runs of a few rows only."""
    d = R.planted_dosages(400, 33, 400)
    x = R.planted_positions(400, 400, step=(1, 1400))
    for mode in (R.IBD1, R.IBD2):
        ref = R.scan(d, x, R.params(mode=mode, **FULL))
        lengths = [s[2] for s in ref["segments"]]
        assert len(lengths) >= 30 and any(15 <= s <= 70 for s in lengths), mode
        counts = ref["n_segments"][np.triu_indices(33, 1)]
        assert len(set(counts.tolist())) >= 3, mode
        assert any(s[3] > 0 for s in ref["segments"]) and any(not ok for *_run, ok in ref["runs"]), mode
        loose = R.scan(d, None, R.params(mode=mode, **LOOSE))
        assert (0, 1, 400, int((d[:, :2] == R.NOT_CALLED).any(axis=1).sum()), 0, 399) in loose["segments"], "one run over everything"
    one, two = R.scan(d, x, R.params(mode=R.IBD1, **FULL)), R.scan(d, x, R.params(mode=R.IBD2, **FULL))
    assert one["sum_sites"].sum() > two["sum_sites"].sum() > 0
    short = R.scan(R.planted_dosages(200, 5, 7, short=True), None, R.params(mode=R.IBD2, min_sites=3, min_length=1, max_gap=0))
    assert sum(3 <= s[2] <= 9 for s in short["segments"]) >= 10
    flat = R.scan(R.uniform_dosages(400, 20, 3), None, R.params(**LOOSE))
    assert max(s[2] for s in flat["segments"]) < 100 and len(flat["segments"]) > 20 * 19 / 2 * 20


@pytest.mark.parametrize("variant", ["bare", "full"])
@pytest.mark.parametrize("mode", [R.IBD1, R.IBD2])
def test_twin_matches_oracle(dev, mode, variant):
    qualifying = 0
    for n in NS:
        for K in KS:
            full = R.planted_dosages(max(K, 1) + 30, 33, 1000 + K)
            pos = R.planted_positions(max(K, 1) + 30, 1000 + K, step=(1, 1400))
            if variant == "bare":
                d, x, p = full[:K, :n], None, R.params(mode=mode, **LOOSE)
            else:                                                                   # a keep mask, positions and every filter
                keep = np.flatnonzero(np.random.default_rng(K).random(K + 30) >= 30 / (K + 30))[:K]
                d, x, p = full[keep][:, :n], pos[keep], R.params(mode=mode, **FULL)
                x = x - x[0] if len(x) else x
            d = np.ascontiguousarray(d)
            ref = R.scan(d, x, p)
            got = dev.ibd_scan_host(d, device_params(dev, p), x=x, capacity=len(ref["segments"]) + 4)
            assert_same(got, ref, (n, K, mode, variant))
            qualifying += len(ref["segments"])
    assert qualifying >= 50


# ---- the twin under sanitizers: a stand-alone program, no sanitizer runtime in this process ---------------------------------------------------
def splitmix_cohort(seed, K, n):
    """The cohort of ferromic_amd/csrc/ibd_host_check.cpp, from the same splitmix64 stream in the same order."""
    mask = (1 << 64) - 1
    s = [seed & mask]

    def rnd():
        s[0] = (s[0] + 0x9E3779B97F4A7C15) & mask
        z = s[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    F = 3
    founder = np.zeros((F, K), dtype=np.uint8)
    for f in range(F):
        for k in range(K):
            founder[f, k] = rnd() % 3
    dosage = np.zeros((K, n), dtype=np.uint8)
    for i in range(n):
        k = 0
        while k < K:
            length = 5 + rnd() % 60
            src = rnd() % (F + 1)
            j = 0
            while j < length and k < K:
                r = rnd() % 1000
                dosage[k, i] = 3 if r < 20 else founder[src, k] if (src < F and r >= 70) else r % 3
                j += 1
                k += 1
    x = np.zeros(K, dtype=np.int64)
    for k in range(K):
        jump = 3000000 if rnd() % 50 == 0 else rnd() % 2000
        x[k] = x[k - 1] + jump if k else rnd() % 1000
    return dosage, x


SANITIZER_CASES = [
    (11, 400, 9, dict(mode=R.IBD1, min_sites=12, min_length=9_000, max_gap=1_000_000, max_bp_per_site=1_500, max_missing=2)),
    (12, 300, 6, dict(mode=R.IBD2, min_sites=5, min_length=1, max_gap=1_000_000, max_bp_per_site=0, max_missing=None)),
    (13, 1, 2, dict(mode=R.IBD1, **LOOSE)),
    (14, 65, 1, dict(mode=R.IBD2, **LOOSE)),                                         # no pair
    (15, 129, 4, dict(mode=R.IBD2, **LOOSE)),
]


def test_twin_under_sanitizers(dev):
    program = os.path.join(BIN_DIR, "ibd_host_check.asan")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    total = 0
    for seed, K, n, kw in SANITIZER_CASES:
        p = R.params(**kw)
        dosage, x = splitmix_cohort(seed, K, n)
        ref = R.scan(dosage, x, p)
        total += len(ref["segments"])
        args = [seed, K, n, p["mode"], p["min_sites"], p["min_length"], p["max_gap"], p["max_bp_per_site"], p["max_missing"]]
        res = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        want = "ibd_host_check: %d kept rows x %d samples, mode %d, %d runs, checksum %016x\n" % (K, n, p["mode"], len(ref["segments"]), R.checksum(ref))
        assert res.stdout == want, (res.stdout, want)
    assert total >= 20
