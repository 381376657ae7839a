"""IBD segments on the device (fmh_ibd_scan) against tests/ibd_ref.py, the oracle written from the definition, and against the host twin
(fmh_ibd_scan_host): every table with array_equal, the segments as sorted lists.  Cohorts are uploaded as bit planes with RANDOM bits under
the uncalled entries (tests/test_gpu_sfs.py's upload): the kernel has to mask them with the called plane.  The output tables are
pre-filled with junk by ferromic_amd.device.ibd_scan: the kernels have to WRITE every entry, the diagonal included.

Shapes are the smallest at which the kernels can go wrong: sample counts around one, two and three edges of the 32-sample pair tile (a
diagonal tile, an off-diagonal tile and tile (0, 3) all occur), a scattered sample list over several tiles, a matrix wider than the
selection; kept-row counts around one and two 64-row words with FMH_IBD_ITEM_ROWS=64, so that every word is a row block of its own and
every run longer than a word is stitched, and 200 rows at the default; pairs designed on the block boundaries; every matrix kind; a keep
mask and a row range inside the matrix; one and three workgroups; a caller's stream; segment buffers that hold every run, two, or none."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import ibd_ref as R
from tests.test_gpu_sfs import KINDS, upload

pytestmark = pytest.mark.gpu

LOOSE = dict(min_sites=1, min_length=1, max_gap=0, max_bp_per_site=0)
FULL = dict(min_sites=12, min_length=9_000, max_gap=1_000_000, max_bp_per_site=1_250, max_missing=2)
MODES = (R.IBD1, R.IBD2)
BLOCK = 64  # FMH_IBD_ITEM_ROWS of most tests


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def device_params(dev, p):
    return dev.ibd_params(mode=p["mode"], min_sites=p["min_sites"], min_length=p["min_length"], max_gap=p["max_gap"],
                          max_bp_per_site=p["max_bp_per_site"], max_missing=None if p["max_missing"] == R.NO_LIMIT else p["max_missing"])


def realise(d, kind, seed, columns=None):
    """(alleles, called or None, dosages as the matrix holds them) of a dosage table in a matrix kind."""
    max_allele, missing = KINDS[kind]
    x, called = R.genotypes_from_dosages(d, seed, columns=columns, high_allele=max_allele, uncalled=missing)
    return x, (called if missing else None), R.dosages(x, called if missing else None)


@functools.lru_cache(maxsize=None)
def cohort(rows, S, kind, seed, flavour="planted"):
    """(alleles [rows][2 S], called or None, dosages [rows][S], positions [rows]) of a cohort that the matrix kind can hold: without a called
    plane a missing genotype is an allele above 1, and a biallelic matrix with nothing missing has no missing genotype."""
    max_allele, missing = KINDS[kind]
    miss = 0.02 if (missing or max_allele > 1) else 0.0
    if flavour == "uniform":
        d = R.uniform_dosages(rows, S, seed, miss=miss)
    else:
        d = R.planted_dosages(rows, S, seed, short=flavour == "short", miss=miss)
    x, called, back = realise(d, kind, seed)
    assert np.array_equal(back, d)
    pos = R.planted_positions(rows, seed, step=(1, 1400))
    for a in (x, called, d, pos):
        if a is not None:
            a.setflags(write=False)
    return x, called, d, pos


def scan_and_check(dev, dm, d, pos, p, what, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, twin=True, stream=None):
    """fmh_ibd_scan with ample capacity against the oracle (and the twin) over the same kept rows and samples; returns (device, oracle)."""
    rows = d.shape[0] - row_begin if row_count is None else row_count
    kept = np.arange(row_begin, row_begin + rows)
    if keep is not None:
        kept = kept[np.asarray(keep, dtype=bool)]
    cols = np.arange(d.shape[1] if n_samples is None else n_samples) if samples is None else np.asarray(samples)
    dosage = np.ascontiguousarray(d[kept][:, cols])
    base = 0 if pos is None or row_begin >= len(pos) else pos[row_begin]
    x = None if pos is None else pos[kept] - base
    ref = R.scan(dosage, x, p)
    # the oracle's rows are kept rows; the device reports rows of the range
    want = [(s[0], s[1], s[2], s[3], int(kept[s[4]] - row_begin), int(kept[s[5]] - row_begin)) for s in ref["segments"]]
    dp = device_params(dev, p)
    positions = None
    if pos is not None:
        positions = np.zeros(dm.variants, dtype=np.uint32)
        positions[row_begin:row_begin + rows] = pos[row_begin:row_begin + rows] - base
    got = dev.ibd_scan(dm, dp, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=row_count, keep=keep, positions=positions,
                       capacity=len(want) + 8, stream=stream)
    for name in R.TABLES:
        assert got.tables[name].dtype == np.uint64 and got.tables[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(got.tables[name], ref[name]), (what, name, np.argwhere(got.tables[name] != ref[name])[:5])
    assert got.count == len(want), (what, got.count, len(want))
    assert R.segment_tuples(got.segments) == want, what
    if twin:
        host = dev.ibd_scan_host(dosage, dp, x=x, capacity=len(want) + 8)
        for name in R.TABLES:
            assert np.array_equal(got.tables[name], host.tables[name]), (what, name, "twin")
        assert R.segment_tuples(host.segments) == ref["segments"], (what, "twin")
    return got, ref


# ---- samples: one, two and three tile edges, a scattered list, a wider matrix --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_sample_counts(dev, fmh_opts, mode):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(200, 97, "missing", 3)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)                           # wider than every selection but the last
    p = R.params(mode=mode, **FULL)
    for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 97):
        got, ref = scan_and_check(dev, dm, d, pos, p, ("samples", n, mode), n_samples=n, twin=n <= 33)
        if n >= 31:
            counts = ref["n_segments"][np.triu_indices(n, 1)]
            assert counts.max() >= 2 and len(set(counts.tolist())) > 1               # the pairs' counts differ
        if n == 97:
            assert ref["n_segments"][:32, 96:].any() and ref["n_segments"][64:96, 64:96].any()   # tile (0, 3) and a late diagonal tile
        if n == 1:
            assert got.count == 0 and got.tables["n_segments"].tolist() == [[0]]


def test_sample_list_over_several_tiles(dev, fmh_opts):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(200, 97, "missing", 3)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    scattered = [0, 1, 3, 17, 31, 32, 40, 63, 64, 90, 95, 96]                       # four tiles of the matrix, twelve of 97
    for mode in MODES:
        got, ref = scan_and_check(dev, dm, d, pos, R.params(mode=mode, **FULL), ("scattered list", mode), samples=scattered)
        assert ref["n_segments"].sum() >= 12
        scan_and_check(dev, dm, d, pos, R.params(mode=mode, **LOOSE), ("two late samples", mode), samples=[70, 96])
    dense = list(range(20, 97, 2))                                                  # 39 samples: two tiles of the selection
    scan_and_check(dev, dm, d, pos, R.params(mode=R.IBD2, **FULL), "every other sample", samples=dense)


# ---- kept rows around one and two words ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["bare", "full"])
@pytest.mark.parametrize("mode", MODES)
def test_kept_rows(dev, fmh_opts, mode, variant):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(1000, 20, "missing", 100)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(mode=mode, **(FULL if variant == "full" else LOOSE))
    segments = 0
    for K in (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1000):
        got, ref = scan_and_check(dev, dm, d, pos if variant == "full" else None, p, (K, mode, variant), n_samples=17, row_count=K)
        segments += got.count
        if K == 0:
            assert got.count == 0 and not any(t.any() for t in got.tables.values())
        if K == 200:  # once more at the default: one block
            fmh_opts.delenv("FMH_IBD_ITEM_ROWS")
            scan_and_check(dev, dm, d, pos if variant == "full" else None, p, (K, mode, variant, "default blocks"), n_samples=17, row_count=K, twin=False)
            fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    assert segments > 0


# ---- a keep mask and a row range inside the matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_row_selection(dev, fmh_opts, mode):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(400, 40, "missing", 7)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(mode=mode, **FULL)
    keep = np.random.default_rng(8).random(300) >= 1 / 3
    got, ref = scan_and_check(dev, dm, d, pos, p, "range", row_begin=37, row_count=300)
    masked, ref_masked = scan_and_check(dev, dm, d, pos, p, "range and keep mask", row_begin=37, row_count=300, keep=keep)
    assert ref["n_segments"].sum() > 0 and ref_masked["n_segments"].sum() > 0 and not np.array_equal(ref["sum_sites"], ref_masked["sum_sites"])
    none, _ = scan_and_check(dev, dm, d, pos, p, "no kept row", row_begin=37, row_count=300, keep=np.zeros(300, dtype=bool))
    assert none.count == 0 and not none.tables["n_segments"].any()
    few = np.zeros(300, dtype=bool)
    few[[5, 80, 290]] = True
    scan_and_check(dev, dm, d, pos, R.params(mode=mode, **LOOSE), "three kept rows", row_begin=37, row_count=300, keep=few)
    scan_and_check(dev, dm, d, pos, p, "an empty range", row_begin=400, row_count=0)


# ---- matrix kinds: with a called plane, with upper allele planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_matrix_kinds(dev, fmh_opts, kind, row_hi):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    max_allele, missing = KINDS[kind]
    x, called, d, pos = cohort(200, 40, kind, 9)
    if missing or max_allele > 1:
        assert (d == R.NOT_CALLED).any()
    for planes in (True, False):
        dm = upload(dev, x, called, max_allele, planes=planes, ploidy=2)
        for mode in MODES:
            got, ref = scan_and_check(dev, dm, d, pos, R.params(mode=mode, **FULL), (kind, planes, mode), twin=planes)
            assert ref["n_segments"].sum() > 0
            if missing or max_allele > 1:
                assert any(s[3] > 0 for s in ref["segments"])                       # a segment with a missing row


# ---- min_sites on the uniform background: many short runs, both sides of 62 ----------------------------------------------------------------------
@pytest.mark.parametrize("min_sites", [1, 62, 63, 64])
def test_min_sites_on_the_uniform_background(dev, fmh_opts, min_sites):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(600, 40, "missing", 41, flavour="uniform")
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    got, ref = scan_and_check(dev, dm, d, None, R.params(mode=R.IBD1, min_sites=min_sites, min_length=1, max_gap=0), ("min_sites", min_sites), twin=min_sites > 1)
    if min_sites == 1:
        assert got.count > 40 * 39 / 2 * 30                                         # dozens of runs per pair
    short = R.scan(d, None, R.params(mode=R.IBD1, **LOOSE)) if min_sites == 62 else None
    if short is not None:
        assert any(s[2] >= 62 for s in short["segments"]) and sum(s[2] < 62 for s in short["segments"]) > 1000


# ---- the grid, a caller's stream, the segment buffer ----------------------------------------------------------------------------------------------
def test_grid_and_stream_do_not_change_a_table(dev, fmh_opts):
    import torch

    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(400, 70, "missing", 11)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(mode=R.IBD1, **FULL)
    base, ref = scan_and_check(dev, dm, d, pos, p, "default grid")
    assert ref["n_segments"].sum() >= 100
    for blocks in ("1", "3"):
        fmh_opts.setenv("FMH_GRID_BLOCKS", blocks)
        scan_and_check(dev, dm, d, pos, p, ("FMH_GRID_BLOCKS", blocks), twin=False)
        fmh_opts.delenv("FMH_IBD_ITEM_ROWS")                                         # the default blocks follow the grid
        scan_and_check(dev, dm, d, pos, p, ("FMH_GRID_BLOCKS", blocks, "default blocks"), twin=False)
        fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    fmh_opts.delenv("FMH_GRID_BLOCKS")
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", "100")                                     # rounded up to 128
    scan_and_check(dev, dm, d, pos, p, "item rows 100", twin=False)
    own = torch.cuda.Stream()
    handle = C.c_void_p(own.cuda_stream)
    assert bool(handle.value), "a stream of its own, not the NULL stream"
    scan_and_check(dev, dm, d, pos, R.params(mode=R.IBD2, **FULL), "a caller's stream", twin=False, stream=handle)


def test_segment_capacity(dev, fmh_opts):
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    x, called, d, pos = cohort(300, 40, "missing", 13)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    p = R.params(mode=R.IBD1, **FULL)
    full, ref = scan_and_check(dev, dm, d, pos, p, "ample capacity")
    truth = set(ref["segments"])
    assert len(truth) == len(ref["segments"]) >= 40
    positions = (pos - pos[0]).astype(np.uint32)
    for capacity in (2, 0):
        got = dev.ibd_scan(dm, device_params(dev, p), positions=positions, capacity=capacity)
        assert got.count == len(truth)                                              # exact, beyond the capacity
        entries = R.segment_tuples(got.segments)
        assert len(entries) == capacity and len(set(entries)) == capacity and set(entries) <= truth
        for name in R.TABLES:
            assert np.array_equal(got.tables[name], full.tables[name])
    counted = dev.ibd_scan(dm, device_params(dev, p), positions=positions)          # no segments asked for
    assert counted.count is None and np.array_equal(counted.tables["n_segments"], ref["n_segments"])
    only = dev.ibd_scan(dm, device_params(dev, p), positions=positions, capacity=len(truth), tables=("sum_length",))   # the other tables NULL
    assert list(only.tables) == ["sum_length"] and np.array_equal(only.tables["sum_length"], ref["sum_length"]) and only.count == len(truth)
    segments_only = dev.ibd_scan(dm, device_params(dev, p), positions=positions, capacity=len(truth), tables=())
    assert R.segment_tuples(segments_only.segments) == ref["segments"]


# ---- blocks: pairs designed on the boundaries of the 64-row blocks ---------------------------------------------------------------------------------
def boundary_cohort():
    """400 kept rows, 16 samples in eight designed pairs (2 p, 2 p + 1): the even sample is hom-ref everywhere, the odd one is hom-alt exactly
    at the DISC rows written here and hom-ref elsewhere.  Positions step by 100 with one gap of 5 Mb that sits on the boundary 256."""
    K = 400
    d = np.zeros((K, 16), dtype=np.uint8)
    disc = {1: [40, 250],            # [41, 249] crosses the boundaries 64, 128 and 192
            3: [63, 128],            # [64, 127] fills block 1 exactly
            5: [100, 192],           # [101, 191] ends on the last row of block 2
            7: [127, 170],           # [128, 169] starts on the first row of block 2
            9: [192, 255],           # a DISC on the first and on the last bit of word 3: [193, 254]
            11: [],                  # no DISC: one run over everything, cut only by the gap on the boundary 256
            13: [],                  # the same with missing rows across the boundary 64
            15: [0, 399]}            # DISC on the first and on the last kept row
    for s, rows in disc.items():
        d[rows, s] = 2
    d[60:70, 13] = R.NOT_CALLED
    pos = np.arange(K, dtype=np.int64) * 100
    pos[256:] += 5_000_000
    return d, pos


def test_block_records_and_stitch(dev, fmh_opts):
    d, pos = boundary_cohort()
    gap = R.params(mode=R.IBD1, min_sites=10, min_length=1, max_gap=1_000_000)
    whole = R.params(mode=R.IBD1, min_sites=10, min_length=1, max_gap=0)
    ref, ref_whole = R.scan(d, pos, gap), R.scan(d, pos, whole)
    # ---- on the oracle alone, before the device is called ----
    def of(r, a, b):
        return [(s[4], s[5], s[3]) for s in r["segments"] if (s[0], s[1]) == (a, b)]
    assert of(ref_whole, 0, 1) == [(0, 39, 0), (41, 249, 0), (251, 399, 0)]          # crosses three block boundaries
    assert of(ref_whole, 2, 3) == [(0, 62, 0), (64, 127, 0), (129, 399, 0)]          # fills a block exactly
    assert of(ref_whole, 4, 5) == [(0, 99, 0), (101, 191, 0), (193, 399, 0)]         # ends on a block's last row
    assert of(ref_whole, 6, 7) == [(0, 126, 0), (128, 169, 0), (171, 399, 0)]        # starts on a block's first row
    assert of(ref_whole, 8, 9) == [(0, 191, 0), (193, 254, 0), (256, 399, 0)]        # DISC on the first and the last bit of a word
    assert of(ref_whole, 10, 11) == [(0, 399, 0)] and of(ref_whole, 12, 13) == [(0, 399, 10)]   # one run over everything
    assert of(ref_whole, 14, 15) == [(1, 398, 0)]
    assert of(ref, 10, 11) == [(0, 255, 0), (256, 399, 0)] and ref["breaks"][256] and ref["breaks"].sum() == 1   # cut by the gap on a boundary
    assert of(ref, 8, 9) == [(0, 191, 0), (193, 254, 0), (256, 399, 0)]               # the gap behind a DISC row
    assert of(ref, 0, 1) == [(0, 39, 0), (41, 249, 0), (256, 399, 0)]                 # [251, 255] is an interior run rejected by min_sites
    # ---- the device: blocks of 64, 128 and the default (one block) ----
    x, called = R.genotypes_from_dosages(d, 22, high_allele=1)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    for item_rows in (str(BLOCK), "128", None):
        if item_rows:
            fmh_opts.setenv("FMH_IBD_ITEM_ROWS", item_rows)
        else:
            fmh_opts.delenv("FMH_IBD_ITEM_ROWS")
        for mode in MODES:
            scan_and_check(dev, dm, d, pos, dict(gap, mode=mode), ("blocks of", item_rows, "gap", mode))
            scan_and_check(dev, dm, d, pos, dict(whole, mode=mode), ("blocks of", item_rows, "no gap", mode))
            scan_and_check(dev, dm, d, None, R.params(mode=mode, **LOOSE), ("blocks of", item_rows, "loose", mode))


# ---- the budget and the refusals --------------------------------------------------------------------------------------------------------------
def test_budget_of_one_byte_is_refused(dev, fmh_opts):
    from ferromic_amd import _abi

    x, called, d, pos = cohort(300, 40, "missing", 13)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    fmh_opts.setenv("FMH_IBD_BUDGET_BYTES", "1")
    with pytest.raises(_abi.FerromicHipError, match="bytes of scratch, above FMH_IBD_BUDGET_BYTES = 1") as err:
        dev.ibd_scan(dm, dev.ibd_params(**LOOSE))
    assert err.value.status == _abi.FMH_ERR_UNSUPPORTED
    assert dev.ibd_scan(dm, dev.ibd_params(**LOOSE), n_samples=1).tables["n_segments"].tolist() == [[0]]   # no pair: no scratch
    fmh_opts.setenv("FMH_IBD_BUDGET_BYTES", "300000")                               # 3 tile pairs x 1 024 slots x 40 B = 120 KiB per block: two blocks fit
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))                                # five blocks do not
    with pytest.raises(_abi.FerromicHipError, match="FMH_IBD_BUDGET_BYTES"):
        dev.ibd_scan(dm, dev.ibd_params(**LOOSE))
    fmh_opts.delenv("FMH_IBD_ITEM_ROWS")                                            # the default takes the blocks the budget leaves
    scan_and_check(dev, dm, d, pos, R.params(mode=R.IBD1, **FULL), "a budget for two blocks", twin=False)


def test_refusals_in_order(dev, fmh_opts):
    """Every refusal of fmh_ibd_scan; each call but the last of a kind is wrong in a LATER way too, so the order shows."""
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called, d, pos = cohort(300, 40, "missing", 13)
    dm = upload(dev, x, called, 1, planes=True, ploidy=2)
    ok, bad_mode = dev.ibd_params(**LOOSE), dev.ibd_params(mode=5, **LOOSE)
    down = np.zeros(300, dtype=np.uint32)
    down[10] = 7
    count = C.c_uint64(0)
    seg = dev.DeviceBuffer(dm.device, 4 * dev.IBD_SEGMENT_DTYPE.itemsize)
    samples = np.array([3, 2], dtype=np.uint32)

    def call(m=dm._h, s=None, n=40, r0=0, rc=300, x_=None, p=ok, out=None, segments=None, cnt=None):
        return lib.fmh_ibd_scan(m, None if s is None else s.ctypes.data, n, r0, rc, None, None if x_ is None else x_.ctypes.data, p, out, segments, 4, cnt, None)

    cases = [
        (lambda: call(m=None, p=None, n=0), b"NULL matrix"),
        (lambda: call(p=None, n=0), b"NULL params"),
        (lambda: call(n=0, s=samples, rc=301), b"n_samples is 0"),
        (lambda: call(n=2, s=samples, rc=301), b"not strictly ascending"),
        (lambda: call(n=41, rc=301), b"exceeds the matrix's 40 samples"),
        (lambda: call(rc=301, p=bad_mode), b"exceed the matrix's 300 variants"),
        (lambda: call(p=bad_mode, x_=down), b"mode"),
        (lambda: call(x_=down), b"descend"),
        (lambda: call(), b"every output is NULL"),
        (lambda: call(segments=seg.ptr), b"h_segment_count"),
    ]
    for make, words in cases:
        assert make() == _abi.FMH_ERR_INVALID and words in lib.fmh_last_error(), (words, lib.fmh_last_error())
    # FMH_ERR_UNSUPPORTED: ploidy, no packed image (each wrong in the budget too), the budget
    fmh_opts.setenv("FMH_IBD_BUDGET_BYTES", "1")
    haploid = upload(dev, np.ascontiguousarray(x[:, :41]), None, 1, planes=True, ploidy=1)
    assert lib.fmh_ibd_scan(haploid._h, None, 2, 0, 300, None, None, ok, None, None, 0, C.byref(count), None) == _abi.FMH_ERR_UNSUPPORTED
    assert b"ploidy 2" in lib.fmh_last_error()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    unpacked = upload(dev, x, None, 1, ploidy=2)
    fmh_opts.delenv("FMH_LAYOUT")
    assert lib.fmh_ibd_scan(unpacked._h, None, 2, 0, 300, None, None, ok, None, None, 0, C.byref(count), None) == _abi.FMH_ERR_UNSUPPORTED
    assert b"fmh_matrix_pack" in lib.fmh_last_error()
    assert call(cnt=C.byref(count)) == _abi.FMH_ERR_UNSUPPORTED and b"FMH_IBD_BUDGET_BYTES" in lib.fmh_last_error()
    fmh_opts.delenv("FMH_IBD_BUDGET_BYTES")
    assert call(cnt=C.byref(count)) == _abi.FMH_OK and count.value > 0
    unpacked.pack()
    assert lib.fmh_ibd_scan(unpacked._h, None, 2, 0, 300, None, None, ok, None, None, 0, C.byref(count), None) == _abi.FMH_OK


# ---- against existing code: kinship's IBS0 counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_sites_and_ibs0_add_up_to_the_kept_rows(dev, fmh_opts, kind):
    """mode IBD1, every filter loose, no gap limit: every row that is not DISC lies in exactly one qualifying run, and a DISC row is an IBS0
    row of fmh_kinship_counts, so sum_sites[i][j] + ibs0[i][j] == K for every pair."""
    fmh_opts.setenv("FMH_IBD_ITEM_ROWS", str(BLOCK))
    max_allele, missing = KINDS[kind]
    x, called, d, pos = cohort(400, 70, kind, 17)
    dm = upload(dev, x, called, max_allele, planes=True, ploidy=2)
    keep = np.random.default_rng(18).random(350) >= 0.25
    K = int(keep.sum())
    got = dev.ibd_scan(dm, dev.ibd_params(mode=dev.IBD1, **LOOSE), n_samples=66, row_begin=20, row_count=350, keep=keep)
    kin = dev.kinship_counts(dm, n_samples=66, row_begin=20, row_count=350, keep=keep)
    assert kin.kept_rows == K and kin.ibs0.any()
    total = got.tables["sum_sites"] + kin.ibs0
    off = ~np.eye(66, dtype=bool)
    assert (total[off] == K).all() and not np.diag(got.tables["sum_sites"]).any()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def assert_result(res, ref, samples, kept, positions, what, mode="ibd1"):
    """An IbdSegments against the oracle's result over the kept rows `kept` (rows in play) of positions `positions`."""
    assert np.array_equal(res.samples, np.asarray(samples, dtype=np.int64)) and res.mode == mode, what
    for field, name in (("n_segments", "n_segments"), ("total_sites", "sum_sites"), ("total_length", "sum_length"), ("longest", "longest_length")):
        got = getattr(res, field)
        assert got.dtype == np.uint64 and got.shape == ref[name].shape and np.array_equal(got, ref[name]), (what, field)
    seg = ref["segments"]
    assert res.kept_rows == len(kept), what
    assert res.segment_a.tolist() == [s[0] for s in seg] and res.segment_b.tolist() == [s[1] for s in seg], what
    assert res.segment_sites.tolist() == [s[2] for s in seg] and res.segment_missing.tolist() == [s[3] for s in seg], what
    assert res.segment_first_row.tolist() == [int(kept[s[4]]) for s in seg] and res.segment_last_row.tolist() == [int(kept[s[5]]) for s in seg], what
    assert res.segment_start.tolist() == [int(positions[kept[s[4]]]) for s in seg], what
    assert res.segment_end.tolist() == [int(positions[kept[s[5]]]) for s in seg], what
    cover = np.zeros(len(positions), dtype=np.uint32)
    for s in seg:
        cover[kept[s[4]]:kept[s[5]] + 1] += 1
    assert res.site_coverage().dtype == np.uint32 and np.array_equal(res.site_coverage(), cover), what
    span = int(positions[kept[-1]] - positions[kept[0]] + 1)
    assert np.array_equal(res.ibd_fraction(), ref["sum_length"].astype(np.float64) / span), what


def test_python_from_numpy_population(fm):
    """1 000 sites x 6 samples of short planted stretches and runs of three sites: hundreds of segments, so the first capacity guess
    (64 + 8 n) overflows and the segments come from a second call."""
    x, called, d, pos = cohort(1000, 6, "missing", 31, flavour="short")
    geno = np.where(called, x, -1).astype(np.int8).reshape(1000, 6, 2)
    whole = [0, 2, 3, 5]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(1, 0)]
    positions = pos + 1000
    pop = fm.Population.from_numpy("p", geno, positions, haps, int(positions[-1]) + 1)
    kw = dict(mode="ibd2", min_sites=3, min_length=1, max_gap=None, max_bp_per_site=None)
    ref = R.scan(d[:, whole], positions, R.params(mode=R.IBD2, min_sites=3, min_length=1, max_gap=0))
    assert len(ref["segments"]) > 64 + 8 * 4                                        # the first guess overflows
    res = pop.ibd_segments(**kw)
    assert isinstance(res, fm.IbdSegments)
    assert_result(res, ref, whole, np.arange(1000), positions, "Population.ibd_segments", mode="ibd2")
    # filters and a sites mask
    sites = np.random.default_rng(32).random(1000) >= 1 / 3
    kept = np.flatnonzero(sites)
    x2, called2, d2, pos2 = cohort(1000, 6, "missing", 33)
    pop2 = fm.Population.from_numpy("q", np.where(called2, x2, -1).astype(np.int8).reshape(1000, 6, 2), pos2, [(s, side) for s in range(6) for side in (0, 1)],
                                    int(pos2[-1]) + 1)
    ref2 = R.scan(d2[kept], pos2[kept], R.params(mode=R.IBD1, **FULL))
    assert ref2["n_segments"].sum() >= 10
    res2 = pop2.ibd_segments(sites=sites, **FULL)
    assert_result(res2, ref2, range(6), kept, pos2, "Population.ibd_segments(sites, filters)")
    tables_only = pop2.ibd_segments(sites=sites, segments=False, **FULL)
    assert np.array_equal(tables_only.n_segments, ref2["n_segments"])
    with pytest.raises(ValueError):
        tables_only.segment_a
    assert pop2.ibd_segments().n_segments.sum() == 0                                 # IBIS's defaults: no run of 436 sites and 7 Mb here


def test_python_variant_list(fm):
    x, called, d, pos = cohort(300, 12, "missing", 35)
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = []
    for i in range(300):
        calls = [None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(12)]
        variants.append(dict(position=int(pos[i]) + 500, genotypes=calls))
    positions = pos + 500
    for mode, name in ((R.IBD1, "ibd1"), (R.IBD2, "ibd2")):
        p = R.params(mode=mode, **FULL)
        ref = R.scan(d, positions, p)
        assert ref["n_segments"].sum() >= 10
        assert_result(fm.ibd_segments(variants, mode=name, **FULL), ref, range(12), np.arange(300), positions, "ibd_segments", mode=name)
    p = R.params(mode=R.IBD1, **FULL)
    samples = [1, 2, 5, 10, 11]
    assert_result(fm.ibd_segments(variants, samples=samples, **FULL), R.scan(d[:, samples], positions, p), samples, np.arange(300), positions,
                  "ibd_segments(samples)")
    wide = np.flatnonzero(np.diff(positions) >= 5) + 1                              # rows with room before them: no position sits on a region bound
    first, end = int(wide[wide >= 40][0]), int(wide[wide >= 250][0])
    lo, hi = int(positions[first]) - 2, int(positions[end - 1]) + 2
    inside = np.arange(first, end)
    sub_d, sub_pos = d[inside], positions[inside]
    sites = np.arange(len(inside)) % 4 != 1
    kept = np.flatnonzero(sites)
    res = fm.ibd_segments(variants, samples=samples, sites=sites, region=(lo, hi), **FULL)
    assert_result(res, R.scan(sub_d[kept][:, samples], sub_pos[kept], p), samples, kept, sub_pos, "ibd_segments(all arguments)")
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(12)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.ibd_segments(haploid)
