"""Runs of homozygosity on the device (fmh_roh_scan) against tests/roh_ref.py, the oracle written from the definition, and against the host
twin (fmh_roh_scan_host): every table with array_equal, the segments as sorted lists.  Cohorts are uploaded as bit planes with RANDOM bits
under the uncalled entries (tests/test_gpu_sfs.py's upload): the kernel has to mask them with the called plane.

Shapes are the smallest at which the kernels can go wrong: sample counts around a 32-bit word of a row (16 samples) and around a sample
group (256), a list of scattered samples over both groups, a matrix wider than the selection; kept-row counts around the window (the two
ends of the range meet), around a step of 64 kept rows, and 200 and 1 000 with FMH_ROH_ITEM_ROWS=64, where a block is no longer than the
halo at W = 64 and a long run crosses several blocks; every matrix kind; a keep mask and a row range inside the matrix; one and three
workgroups; segment buffers that hold every run, two, or none."""

import functools

import numpy as np
import pytest

from tests import roh_ref as R
from tests.test_gpu_sfs import KINDS, upload

pytestmark = pytest.mark.gpu

WINDOWS = (1, 2, 5, 50, 64)
LOOSE = dict(min_sites=1, min_length=1, max_gap=0, max_bp_per_site=0)
FULL = dict(window_het=1, window_missing=2, threshold=0.05, min_sites=12, min_length=12_000, max_gap=1_000_000, max_bp_per_site=1_250, max_het=2,
            max_missing=2, bin_edges=(15_000, 25_000, 50_000))
BLOCK = 64  # FMH_ROH_ITEM_ROWS of most tests


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def device_params(dev, p):
    return dev.roh_params(window=p["window"], window_het=p["window_het"], window_missing=p["window_missing"], need=np.array(p["need"], dtype=np.uint8),
                          min_sites=p["min_sites"], min_length=p["min_length"], max_gap=p["max_gap"], max_bp_per_site=p["max_bp_per_site"],
                          max_het=None if p["max_het"] == R.NO_LIMIT else p["max_het"],
                          max_missing=None if p["max_missing"] == R.NO_LIMIT else p["max_missing"], bin_edges=p["bin_edges"])


@functools.lru_cache(maxsize=None)
def cohort(rows, S, kind, seed, short=False):
    """(alleles [rows][2 S], called or None, states [rows][S], positions [rows]) of a planted cohort that the matrix kind can hold: without
    a called plane a missing genotype is an allele above 1, and a biallelic matrix with nothing missing has no MISS state."""
    max_allele, missing = KINDS[kind]
    stretch = dict(stretch=(3, 9), outside=(2, 6)) if short else dict(stretch=(15, 70), outside=(8, 40))
    st = R.planted_states(rows, S, seed, miss=0.02 if (missing or max_allele > 1) else 0.0, **stretch)
    x, called = R.genotypes_from_states(st, seed, high_allele=max_allele, uncalled=missing)
    assert np.array_equal(R.states(x, called), st)
    pos = R.planted_positions(rows, seed, step=(1, 1400))
    for a in (x, called, st, pos):
        a.setflags(write=False)
    return x, (called if missing else None), st, pos


def scan_and_check(dev, dm, st, pos, p, what, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, twin=True):
    """fmh_roh_scan with ample capacity against the oracle (and the twin) over the same kept rows and samples; returns (device, oracle)."""
    rows = st.shape[0] - row_begin if row_count is None else row_count
    kept = np.arange(row_begin, row_begin + rows)
    if keep is not None:
        kept = kept[np.asarray(keep, dtype=bool)]
    cols = np.arange(st.shape[1] if n_samples is None else n_samples) if samples is None else np.asarray(samples)
    state = np.ascontiguousarray(st[kept][:, cols])
    base = 0 if pos is None or row_begin >= len(pos) else pos[row_begin]
    x = None if pos is None else pos[kept] - base
    ref = R.scan(state, x, p)
    # the oracle's rows are kept rows; the device reports rows of the range
    want = [(s[0], s[1], s[2], s[3], int(kept[s[4]] - row_begin), int(kept[s[5]] - row_begin)) for s in ref["segments"]]
    dp = device_params(dev, p)
    positions = None
    if pos is not None:
        positions = np.zeros(dm.variants, dtype=np.uint32)
        positions[row_begin:row_begin + rows] = pos[row_begin:row_begin + rows] - base
    got = dev.roh_scan(dm, dp, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=row_count, keep=keep, positions=positions,
                       capacity=len(want) + 8)
    for name in R.TABLES + ("bin_runs", "bin_length"):
        assert got.tables[name].dtype == np.uint64 and got.tables[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(got.tables[name], ref[name]), (what, name, got.tables[name], ref[name])
    assert got.count == len(want), (what, got.count, len(want))
    assert R.segment_tuples(got.segments) == want, what
    if twin:
        host = dev.roh_scan_host(state, dp, x=x, capacity=len(want) + 8)
        for name in R.TABLES + ("bin_runs", "bin_length"):
            assert np.array_equal(got.tables[name], host.tables[name]), (what, name, "twin")
        assert R.segment_tuples(host.segments) == ref["segments"], (what, "twin")
    return got, ref


# ---- samples: a word, a group, a scattered list, a wider matrix ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 15, 16, 17, 255, 256, 257])
def test_sample_counts(dev, fmh_opts, S):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    x, called, st, pos = cohort(200, S, "missing", 3)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    got, ref = scan_and_check(dev, dm, st, pos, R.params(window=5, **FULL), ("samples", S))
    if S >= 15:
        assert ref["n_runs"].max() >= 2 and len(set(ref["n_runs"].tolist())) > 1      # the samples' n_runs differ


def test_sample_list_and_wider_matrix(dev, fmh_opts):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    x, called, st, pos = cohort(200, 300, "multi3-missing", 4)
    dm = upload(dev, x, called, 3, planes=True, ploidy=2)
    p = R.params(window=5, **FULL)
    scattered = [3, 17, 64, 255, 256, 271, 299]                                     # both sample groups, seven of 300
    got, ref = scan_and_check(dev, dm, st, pos, p, "scattered list", samples=scattered)
    assert ref["n_runs"].sum() >= 7
    scan_and_check(dev, dm, st, pos, p, "three samples more than selected", n_samples=297)
    scan_and_check(dev, dm, st, pos, p, "one sample of the second group", samples=[260])
    scan_and_check(dev, dm, st, pos, p, "the first sample", n_samples=1)


# ---- kept rows around the window and the step, every window ---------------------------------------------------------------------------------
def kept_rows_of(W):
    return sorted({0, W - 1, W, W + 1, 2 * W - 2, 2 * W - 1, 63, 64, 65, 200, 1000})


@pytest.mark.parametrize("variant", ["bare", "full"])
@pytest.mark.parametrize("W", WINDOWS)
def test_kept_rows_and_windows(dev, fmh_opts, W, variant):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    p = R.params(window=W, **FULL) if variant == "full" else R.params(window=W, window_het=1, window_missing=2, threshold=0.05, **LOOSE)
    runs = 0
    for K in kept_rows_of(W):
        if K == 0:
            continue  # a matrix has a row; no kept row is test_row_selection's keep mask
        x, called, st, pos = cohort(K, 20, "missing", 100 + W)
        dm = upload(dev, x, called, 1, planes=True, ploidy=2)
        got, ref = scan_and_check(dev, dm, st, pos if variant == "full" else None, p, (W, K, variant), n_samples=17)
        runs += got.count
        if K < W:
            assert got.count == 0 and not got.tables["n_runs"].any()
        if K == 1000:  # once more at the default: one block
            fmh_opts.delenv("FMH_ROH_ITEM_ROWS")
            scan_and_check(dev, dm, st, pos if variant == "full" else None, p, (W, K, variant, "one block"), n_samples=17, twin=False)
            fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    assert runs > 0


# ---- a keep mask and a row range inside the matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [5, 64])
def test_row_selection(dev, fmh_opts, W):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    x, called, st, pos = cohort(400, 40, "missing", 7)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(window=W, **FULL) if W == 5 else R.params(window=W, **{**FULL, "window_het": 5, "window_missing": 4, "max_het": 10, "max_missing": 10})
    keep = np.random.default_rng(8).random(300) >= 1 / 3
    got, ref = scan_and_check(dev, dm, st, pos, p, "range", row_begin=37, row_count=300)
    masked, ref_masked = scan_and_check(dev, dm, st, pos, p, "range and keep mask", row_begin=37, row_count=300, keep=keep)
    assert ref["n_runs"].sum() > 0 and ref_masked["n_runs"].sum() > 0 and not np.array_equal(ref["sum_sites"], ref_masked["sum_sites"])
    none, _ = scan_and_check(dev, dm, st, pos, p, "no kept row", row_begin=37, row_count=300, keep=np.zeros(300, dtype=bool))
    assert none.count == 0 and not none.tables["n_runs"].any() and not none.tables["bin_runs"].any()
    few = np.zeros(300, dtype=bool)
    few[[5, 80, 290]] = True
    scan_and_check(dev, dm, st, pos, R.params(window=2, window_het=0, window_missing=0, threshold=0.0, **LOOSE), "three kept rows", row_begin=37,
                   row_count=300, keep=few)
    scan_and_check(dev, dm, st, pos, p, "an empty range", row_begin=400, row_count=0)


# ---- matrix kinds: with a called plane, with upper allele planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", None], ids=["row_hi=0", "row_hi=default"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_matrix_kinds(dev, fmh_opts, kind, row_hi):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    if row_hi is not None:
        fmh_opts.setenv("FMH_ROW_HI", row_hi)
    max_allele, missing = KINDS[kind]
    x, called, st, pos = cohort(200, 40, kind, 9)
    if missing or max_allele > 1:
        assert (st == R.MISS).any()
    for planes in (True, False):
        dm = upload(dev, x, called, max_allele, planes=planes, ploidy=2)
        for W in (5, 50):
            got, ref = scan_and_check(dev, dm, st, pos, R.params(window=W, **FULL), (kind, planes, W), twin=planes)
            assert ref["n_runs"].sum() > 0


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------------
def test_grid_does_not_change_a_table(dev, fmh_opts):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    x, called, st, pos = cohort(1000, 300, "missing", 11)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(window=50, **FULL)
    base, ref = scan_and_check(dev, dm, st, pos, p, "default grid")
    assert ref["n_runs"].sum() >= 100
    for blocks in ("1", "3"):
        fmh_opts.setenv("FMH_GRID_BLOCKS", blocks)
        got, _ = scan_and_check(dev, dm, st, pos, p, ("FMH_GRID_BLOCKS", blocks), twin=False)
        for name in base.tables:
            assert np.array_equal(got.tables[name], base.tables[name]), (blocks, name)
    fmh_opts.delenv("FMH_GRID_BLOCKS")
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", "100")                                     # rounded up to 128
    scan_and_check(dev, dm, st, pos, p, "item rows 100", twin=False)


# ---- segments: every run, two, none ---------------------------------------------------------------------------------------------------------
def test_segment_capacity(dev, fmh_opts):
    fmh_opts.setenv("FMH_ROH_ITEM_ROWS", str(BLOCK))
    x, called, st, pos = cohort(300, 40, "missing", 13)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(window=5, **FULL)
    full, ref = scan_and_check(dev, dm, st, pos, p, "ample capacity")
    truth = set(ref["segments"])
    assert len(truth) == len(ref["segments"]) >= 40
    positions = (pos - pos[0]).astype(np.uint32)
    for capacity in (2, 0):
        got = dev.roh_scan(dm, device_params(dev, p), positions=positions, capacity=capacity)
        assert got.count == len(truth)                                              # exact, beyond the capacity
        entries = R.segment_tuples(got.segments)
        assert len(entries) == capacity and len(set(entries)) == capacity and set(entries) <= truth
        for name in base_tables(full):
            assert np.array_equal(got.tables[name], full.tables[name])
    counted = dev.roh_scan(dm, device_params(dev, p), positions=positions)          # no segments asked for
    assert counted.count is None and np.array_equal(counted.tables["n_runs"], ref["n_runs"])


def base_tables(result):
    return list(result.tables)


# ---- blocks: runs that cross, fill, end at and are cut at block boundaries ------------------------------------------------------------------------
def boundary_cohort():
    """1 000 kept rows, 24 samples; W = 5, no het and no missing call in a window, need 1: a run is exactly a HOM stretch of at least five
    rows.  Samples 0..5 are designed on the blocks of 64 kept rows, the others planted."""
    K, S = 1000, 24
    st = np.array(R.planted_states(K, S, 21, stretch=(15, 70), outside=(8, 40)))
    st[:, :6] = R.HET
    st[70:400, 0] = R.HOM            # crosses the boundaries 128, 192, 256, 320, 384; blocks 2..5 lie wholly inside it
    st[150:192, 1] = R.HOM           # ends exactly at the last row of block 2; block 3 starts outside a run
    st[600:700, 2] = R.HOM           # cut by the gap that sits on the boundary 640
    st[10:13, 3] = R.HOM             # too short for a window
    st[20:28, 3] = R.HOM             # an interior run of 8 sites: rejected by min_sites = 10
    st[200:230, 3] = R.HOM           # an interior run that qualifies
    st[0:100, 4] = R.HOM             # touches the first kept row
    st[900:1000, 5] = R.HOM          # touches the last kept row
    pos = np.arange(K, dtype=np.int64) * 100
    pos[640:] += 5_000_000
    return st, pos


def test_block_records_and_stitch(dev, fmh_opts):
    st, pos = boundary_cohort()
    p = R.params(window=5, window_het=0, window_missing=0, threshold=0.0, min_sites=10, min_length=1, max_gap=1_000_000, max_bp_per_site=0)
    ref = R.scan(st, pos, p)
    # ---- on the oracle alone, before the device is called ----
    runs = ref["runs"]
    assert any(last // BLOCK - first // BLOCK >= 3 for (_, first, last, *_rest) in runs), "a run crosses three block boundaries"
    assert any(first <= BLOCK * b and last >= BLOCK * b + BLOCK - 1 for (_, first, last, *_rest) in runs for b in range(1000 // BLOCK)), "a block inside a run"
    assert any(last % BLOCK == BLOCK - 1 and not ref["in_run"][last + 1, i] for (i, first, last, *_rest) in runs if last + 1 < 1000), "a run ends with its block"
    assert any(ref["breaks"][k] and ref["in_run"][k - 1, i] and ref["in_run"][k, i] for k in range(BLOCK, 1000, BLOCK) for i in range(6)), "a gap on a boundary"
    assert any(first // BLOCK == last // BLOCK and first % BLOCK and last % BLOCK != BLOCK - 1 and last - first + 1 < p["min_sites"] and not ok
               for (_, first, last, _h, _m, _l, ok) in runs), "an interior run rejected by min_sites"
    assert any(first == 0 for (_, first, *_rest) in runs) and any(last == 999 for (_, _f, last, *_rest) in runs)
    assert len(set(ref["n_runs"].tolist())) > 2
    assert [s for s in ref["segments"] if s[0] < 6] == [(0, 330, 0, 0, 70, 399), (1, 42, 0, 0, 150, 191), (2, 40, 0, 0, 600, 639), (2, 60, 0, 0, 640, 699),
                                                        (3, 30, 0, 0, 200, 229), (4, 100, 0, 0, 0, 99), (5, 100, 0, 0, 900, 999)]
    # ---- the device: blocks of 64, 128 and 4 096 (one block) kept rows ----
    x, called = R.genotypes_from_states(st, 22, high_allele=1)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    for item_rows in (str(BLOCK), "128", None):
        if item_rows:
            fmh_opts.setenv("FMH_ROH_ITEM_ROWS", item_rows)
        else:
            fmh_opts.delenv("FMH_ROH_ITEM_ROWS")
        scan_and_check(dev, dm, st, pos, p, ("blocks of", item_rows))
        scan_and_check(dev, dm, st, pos, R.params(window=64, window_het=2, window_missing=2, threshold=0.05, **LOOSE), ("blocks of", item_rows, "W = 64"))


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def assert_result(res, ref, samples, kept, positions, what):
    """A HomozygosityRuns against the oracle's result over the kept rows `kept` (rows in play) of positions `positions`."""
    assert np.array_equal(res.samples, np.asarray(samples, dtype=np.int64)), what
    for field, name in (("n_runs", "n_runs"), ("total_sites", "sum_sites"), ("total_length", "sum_length"), ("longest", "longest_length"),
                        ("bin_runs", "bin_runs"), ("bin_length", "bin_length")):
        got = getattr(res, field)
        assert got.dtype == np.uint64 and got.shape == ref[name].shape and np.array_equal(got, ref[name]), (what, field)
    seg = ref["segments"]
    assert res.kept_rows == len(kept), what
    assert res.segment_sample.tolist() == [s[0] for s in seg] and res.segment_sites.tolist() == [s[1] for s in seg], what
    assert res.segment_het.tolist() == [s[2] for s in seg] and res.segment_missing.tolist() == [s[3] for s in seg], what
    assert res.segment_first_row.tolist() == [int(kept[s[4]]) for s in seg] and res.segment_last_row.tolist() == [int(kept[s[5]]) for s in seg], what
    assert res.segment_start.tolist() == [int(positions[kept[s[4]]]) for s in seg], what
    assert res.segment_end.tolist() == [int(positions[kept[s[5]]]) for s in seg], what
    cover = np.zeros(len(positions), dtype=np.uint32)
    for s in seg:
        cover[kept[s[4]]:kept[s[5]] + 1] += 1
    assert res.site_coverage().dtype == np.uint32 and np.array_equal(res.site_coverage(), cover), what
    span = int(positions[kept[-1]] - positions[kept[0]] + 1)
    assert np.array_equal(res.f_roh(), ref["sum_length"].astype(np.float64) / span), what


def test_python_from_numpy_population(fm):
    """1 000 sites x 5 samples of short planted stretches; W = 2 and runs of two sites: hundreds of runs, so the first capacity guess
    (64 + 8 n) overflows and the segments come from a second call."""
    x, called, st, pos = cohort(1000, 5, "missing", 31, short=True)
    geno = np.where(called, x, -1).astype(np.int8).reshape(1000, 5, 2)
    whole = [0, 2, 4]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(1, 0)]
    positions = pos + 1000
    pop = fm.Population.from_numpy("p", geno, positions, haps, int(positions[-1]) + 1)
    kw = dict(window=2, window_het=0, window_missing=0, window_threshold=0.05, min_sites=2, min_length=1, max_gap=None, max_bp_per_site=None)
    p = R.params(window=2, window_het=0, window_missing=0, threshold=0.05, min_sites=2, min_length=1, max_gap=0, max_bp_per_site=0)
    ref = R.scan(st[:, whole], positions, p)
    assert len(ref["segments"]) > 64 + 8 * 3                                        # the first guess overflows
    res = pop.runs_of_homozygosity(**kw)
    assert isinstance(res, fm.HomozygosityRuns)
    assert_result(res, ref, whole, np.arange(1000), positions, "Population.runs_of_homozygosity")
    # PLINK-like filters, bins and a sites mask
    sites = np.random.default_rng(32).random(1000) >= 1 / 3
    kept = np.flatnonzero(sites)
    x2, called2, st2, pos2 = cohort(1000, 5, "missing", 33)
    pop2 = fm.Population.from_numpy("q", np.where(called2, x2, -1).astype(np.int8).reshape(1000, 5, 2), pos2, [(s, side) for s in range(5) for side in (0, 1)],
                                    int(pos2[-1]) + 1)
    p2 = R.params(window=5, **FULL)
    ref2 = R.scan(st2[kept], pos2[kept], p2)
    assert ref2["n_runs"].sum() >= 5
    res2 = pop2.runs_of_homozygosity(sites=sites, window=5, window_het=1, window_missing=2, window_threshold=0.05, min_sites=12, min_length=12_000,
                                     max_gap=1_000_000, max_bp_per_site=1_250, max_het=2, max_missing=2, length_bins=[15_000, 25_000, 50_000])
    assert_result(res2, ref2, range(5), kept, pos2, "Population.runs_of_homozygosity(sites, filters, bins)")
    tables_only = pop2.runs_of_homozygosity(sites=sites, window=5, window_het=1, window_missing=2, min_sites=12, min_length=12_000, max_bp_per_site=1_250,
                                            max_het=2, max_missing=2, segments=False)
    assert np.array_equal(tables_only.n_runs, ref2["n_runs"])
    with pytest.raises(ValueError):
        tables_only.segment_sample


def test_python_variant_list(fm):
    x, called, st, pos = cohort(300, 12, "missing", 35)
    st = np.array(st)
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = []
    for i in range(300):
        calls = [None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(12)]
        variants.append(dict(position=int(pos[i]) + 500, genotypes=calls))
    positions = pos + 500
    kw = dict(window=5, window_het=1, window_missing=2, window_threshold=0.05, min_sites=12, min_length=12_000, max_gap=1_000_000, max_bp_per_site=1_250,
              max_het=2, max_missing=2, length_bins=[15_000, 25_000, 50_000])
    p = R.params(window=5, **FULL)
    ref = R.scan(st, positions, p)
    assert ref["n_runs"].sum() >= 10
    assert_result(fm.runs_of_homozygosity(variants, **kw), ref, range(12), np.arange(300), positions, "runs_of_homozygosity")
    samples = [1, 2, 5, 10, 11]
    assert_result(fm.runs_of_homozygosity(variants, samples=samples, **kw), R.scan(st[:, samples], positions, p), samples, np.arange(300), positions,
                  "runs_of_homozygosity(samples)")
    wide = np.flatnonzero(np.diff(positions) >= 5) + 1                              # rows with room before them: no position sits on a region bound
    first, end = int(wide[wide >= 40][0]), int(wide[wide >= 250][0])
    lo, hi = int(positions[first]) - 2, int(positions[end - 1]) + 2
    inside = np.arange(first, end)
    sub_st, sub_pos = st[inside], positions[inside]
    sites = np.arange(len(inside)) % 4 != 1
    kept = np.flatnonzero(sites)
    res = fm.runs_of_homozygosity(variants, samples=samples, sites=sites, region=(lo, hi), **kw)
    assert_result(res, R.scan(sub_st[kept][:, samples], sub_pos[kept], p), samples, kept, sub_pos, "runs_of_homozygosity(all arguments)")
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(12)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.runs_of_homozygosity(haploid)
