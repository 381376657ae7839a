"""Extended haplotype homozygosity scans on the device (fmh_ehh_scan) against tests/ehh_ref.py, the numpy oracle written from the definition.
Every comparison is array_equal on integers: the records of both sides, the curve of pair counts, and the same outputs again under every
launch shape (threads per workgroup, row tables built (FMH_ROW_HI=2, or 4 096 rows and more) or not, a grid smaller than the item count, a
caller's stream).

Cohorts are founder mosaics built in numpy (columns drawn independently agree over a handful of rows only, so nothing would walk far), with
the missing calls and upper alleles of the four cohort kinds of tests/test_gpu_hap.py laid over them.  Shapes are the smallest at which each
part of the kernel can go wrong: groups of 1, 2, 3 members (a core of 0, 1, 2), around one wave, more members than a workgroup has threads,
sparse groups over a partial and over many 128-byte lines, a partition whose bitmap is longer than one wave's pass of the scan, the largest
group the kernel takes; focal rows at both ends of a range strictly inside the matrix; max_extent of 1 and of exactly the distance to the
edge; a case worked by hand whose threshold test is an equality; more items than the grid has workgroups."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import ehh_ref
from tests.test_gpu_sfs import KINDS, upload

pytestmark = pytest.mark.gpu

FIELDS = ("area2", "pair_steps", "steps", "core", "flags", "reserved")
EDGES = ehh_ref.EDGE0 | ehh_ref.EDGE1
GAPS = ehh_ref.GAP0 | ehh_ref.GAP1


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


# ---- cohorts ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mosaic_cohort(rows, cols, kind, seed=0, founders=6, switch=0.02, mutation=0.004):
    """(alleles [rows][cols] uint8, called [rows][cols] bool or None, positions [rows] uint32), read-only and shared between the tests: a
    founder mosaic with the upper alleles and the missing calls of `kind` on a third of the rows each."""
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7919 * rows + 31 * cols + 1000003 * seed + max_allele + missing)
    x = ehh_ref.mosaic(rows, cols, founders, switch, mutation, seed=int(rng.integers(1 << 30))).copy()
    if max_allele > 1:
        some = rng.random(rows) < 1 / 3
        high = (x == 1) & some[:, None] & (rng.random((rows, cols)) < 0.05)
        x[high] = rng.integers(2, max_allele + 1, size=int(high.sum()), dtype=np.uint8)
        whole = rng.random(rows) < 0.05  # rows whose carriers all hold an upper allele: no core 1 there
        x[whole] = np.where(x[whole] == 1, max_allele, x[whole])
    called = None
    if missing:
        some = rng.random(rows) < 1 / 3
        called = ~(some[:, None] & (rng.random((rows, cols)) < 0.03))
        if rows > 9:
            called[9] = False  # one all-uncalled row: nobody is in a core, and as a flank it splits nothing
        called.setflags(write=False)
    positions = np.cumsum(rng.integers(0, 1000, size=rows)).astype(np.uint32)
    x.setflags(write=False)
    positions.setflags(write=False)
    return x, called, positions


PROTOTYPE_FOCAL = range(0, 400, 3)
PROTOTYPE_CURVE_FOCAL = range(0, 400, 8)


@functools.lru_cache(maxsize=None)
def prototype_mosaic():
    """The cohort of the issue's prototype: 6 founders, 96 columns, 400 rows, switch 0.01 per row, mutation 0.002 - and its oracle over every
    third focal row at threshold 1 / 20, and over every eighth with the curve up to 230 rows, computed once."""
    x = ehh_ref.mosaic(400, 96, founders=6, switch=0.01, mutation=0.002, seed=2024)
    x.setflags(write=False)
    mask = np.ones(96, dtype=bool)
    sides, _ = ehh_ref.scan(x, None, mask, PROTOTYPE_FOCAL, min_ehh=(1, 20))
    capped, pairs = ehh_ref.scan(x, None, mask, PROTOTYPE_CURVE_FOCAL, min_ehh=(1, 20), max_extent=230, curve=True)
    for a in (sides, capped, pairs):
        a.setflags(write=False)
    return x, mask, sides, capped, pairs


def run(dev, dm, mask, focal, **kw):
    g = dev.Groups(dm, np.asarray(mask)[None, :].astype(np.uint8))
    try:
        return dev.ehh_scan(dm, g, focal, **kw)
    finally:
        g.close()


def assert_equal(got, ref, what):
    ref_sides, ref_pairs = ref
    assert got.sides.shape == ref_sides.shape, what
    for field in FIELDS:
        assert np.array_equal(got.sides[field], ref_sides[field]), (what, field)
    if ref_pairs is None:
        assert got.pairs is None, what
    else:
        assert got.pairs.dtype == np.uint32 and np.array_equal(got.pairs, ref_pairs), what


def check(dev, dm, x, called, mask, focal, what, **kw):
    """One call against the oracle with the same arguments; returns the oracle's records."""
    curve = kw.pop("curve", False)
    ref = ehh_ref.scan(x, called, mask, focal, curve=curve, **kw)
    assert_equal(run(dev, dm, mask, focal, curve=curve, fill=0xC3, **kw), ref, what)
    return ref[0]


# ---- group sizes x matrix kinds x row tables ------------------------------------------------------------------------------------------
def sparse_mask(cols, members, seed):
    rng = np.random.default_rng(cols + seed)
    mask = np.zeros(cols, dtype=bool)
    mask[rng.choice(cols - 1, size=members - 1, replace=False)] = True
    mask[cols - 1] = True
    return mask


@pytest.mark.parametrize("row_hi", ["0", "2", None], ids=["row_hi=0", "row_hi=2", "row_hi=default"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_group_size_and_cohort_kind(dev, fmh_opts, kind, row_hi):
    """FMH_ROW_HI=2 builds the row tables (row_gap: rows with an uncalled entry, row_hi: rows with an allele above 1) at any size, 0 builds
    none, and the default builds none below 4 096 rows: with the tables the kernel skips the called and the upper planes of the rows that
    do not need them - at the focal row, in the row loop and in the line fetch of either direction."""
    rows = 120
    focal = sorted(set(range(0, rows, 7)) | {9, rows - 1})
    if row_hi is not None:
        fmh_opts.setenv("FMH_ROW_HI", row_hi)  # read when the matrix is made
    max_allele, missing = KINDS[kind]
    seen = dict(edge=0, normal=0, neither=0, long=0)
    for cols in (1, 2, 3, 63, 64, 65, 257, 70, 4100):
        x, called, positions = mosaic_cohort(rows, cols, kind)
        masks = {"all": np.ones(cols, dtype=bool)}
        if cols == 257:
            masks["every-second"] = np.arange(cols) % 2 == 0
        if cols in (70, 4100):
            masks = {"sparse": sparse_mask(cols, 9 if cols == 70 else 41, 3)}
        dm = upload(dev, x, called, max_allele, planes=True)
        try:
            for name, mask in masks.items():
                sides = check(dev, dm, x, called, mask, focal, (kind, row_hi, cols, name), positions=positions, min_ehh=(1, 20))
                check(dev, dm, x, called, mask, focal[::3], (kind, row_hi, cols, name, "unit"), max_extent=25, curve=True)
                seen["edge"] += int((sides["flags"] & EDGES != 0).sum())
                seen["normal"] += int(((sides["flags"] == 0) & (sides["steps"].max(axis=2) > 0)).sum())
                seen["neither"] += int((sides["core"].sum(axis=2) < mask.sum()).sum())
                seen["long"] += int((sides["steps"] > 40).sum())
        finally:
            dm.close()
    # not vacuous (from the oracle): scans that met the edge, scans that ended at the threshold, members of neither core, long walks
    assert seen["edge"] > 0 and seen["normal"] > 20 and seen["long"] > 0
    assert (seen["neither"] > 0) == (missing or max_allele > 1)


# ---- wide partitions ------------------------------------------------------------------------------------------------------------------
def test_labels_above_2048_under_every_thread_count(dev, fmh_opts):
    """2 100 members drawn independently at frequency 0.5, no threshold: a scan goes on until every member of both cores is its own class, so
    K passes 2 048 and the bitmap of 2 K bits is 132 words - more than the 64 threads of the smallest workgroup scan in one go."""
    rows, cols = 72, 2100
    x = np.random.default_rng(5).integers(0, 2, size=(rows, cols), dtype=np.uint8)
    mask = np.ones(cols, dtype=bool)
    focal = [0, 36, 71]
    ref = ehh_ref.scan(x, None, mask, focal, max_extent=30, curve=True)
    assert (ref[0]["flags"][1] == 0).all() and ref[0]["steps"][1].min() >= 10  # ended by P = 0: everyone distinct
    dm = upload(dev, x, None, 1, planes=True)
    try:
        for threads in (None,) + dev.HAP_THREADS:
            if threads is not None:
                fmh_opts.setenv("FMH_HAP_THREADS", threads)
            assert_equal(run(dev, dm, mask, focal, max_extent=30, curve=True, fill=0x5A), ref, threads)
    finally:
        dm.close()


def test_the_largest_group_and_one_member_more(dev):
    from ferromic_amd import _abi
    from tests.test_gpu_hap import largest_cohort

    cap = dev.ehh_max_members()
    x = largest_cohort(cap)  # 24 rows; every haplotype of the first half has a twin in the second
    mask = np.ones(cap + 1, dtype=bool)
    mask[cap // 3] = False  # exactly `cap` members
    focal = [0, 12, 23]
    dm = upload(dev, x, None, 1, planes=True, ploidy=1)
    try:
        sides = check(dev, dm, x, None, mask, focal, "cap")
        assert sides["core"].sum(axis=2).min() == cap and (sides["flags"] & EDGES).any() and sides["pair_steps"].max() > 2**26
        with pytest.raises(_abi.FerromicHipError) as err:
            run(dev, dm, np.ones(cap + 1, dtype=bool), focal)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and str(cap) in str(err.value)
    finally:
        dm.close()


# ---- ranges, extents, stop rules --------------------------------------------------------------------------------------------------------
def test_a_range_strictly_inside_the_matrix(dev):
    """Focal rows at the first and the last row of the range and next to them; scans stop at the range (EDGE) although the matrix goes on.
    max_extent of 1, and of exactly the distance from a focal row to the end of the range."""
    rows, cols = 300, 65
    x, called, positions = mosaic_cohort(rows, cols, "multi3-missing", seed=4, switch=0.01, mutation=0.002)
    mask = np.ones(cols, dtype=bool)
    begin, end = 40, 260
    focal = [begin, begin + 1, 150, end - 2, end - 1]
    dm = upload(dev, x, called, 3, planes=True)
    try:
        sides = check(dev, dm, x, called, mask, focal, "inside", row_begin=begin, row_end=end, positions=positions, min_ehh=(1, 50))
        assert (sides["steps"][0, 0] == 0).all() and (sides["steps"][4, 1] == 0).all()  # nowhere to go
        assert (sides["steps"][1, 0] <= 1).all() and sides["steps"][2].max() > 30
        whole = ehh_ref.scan(x, called, mask, focal, positions=positions, min_ehh=(1, 50))[0]
        assert not np.array_equal(whole["steps"], sides["steps"]), "the range cut no scan short"
        one = check(dev, dm, x, called, mask, focal, "max_extent=1", row_begin=begin, row_end=end, max_extent=1, curve=True)
        assert one["steps"].max() == 1
        for f in (150, 200):
            to_edge = end - 1 - f
            exact = check(dev, dm, x, called, mask, [f], ("to the edge", f), row_begin=begin, row_end=end, max_extent=to_edge, curve=True, min_ehh=(0, 1))
            beyond = check(dev, dm, x, called, mask, [f], ("past the edge", f), row_begin=begin, row_end=end, max_extent=to_edge + 1, min_ehh=(0, 1))
            assert np.array_equal(exact["steps"][0, 1], beyond["steps"][0, 1])
    finally:
        dm.close()


def test_the_case_worked_by_hand(dev):
    """3 rows x 8 columns: P(1) den == P(0) num exactly (the step counts), one hundredth above it stops; a zero gap and an area beyond 2^34."""
    from tests.test_ehh_cpu import hand_made

    x, positions = hand_made()
    mask = np.ones(8, dtype=bool)
    dm = upload(dev, x, None, 3, planes=True)
    try:
        g = dev.Groups(dm, mask[None, :].astype(np.uint8))
        got = dev.ehh_scan(dm, g, [0], positions=positions, min_ehh=(1, 10), max_extent=2, curve=True, fill=0xFF)
        assert_equal(got, ehh_ref.scan(x, None, mask, [0], positions=positions, min_ehh=(1, 10), max_extent=2, curve=True), "1/10")
        right = got.sides[0, 1]
        assert right["core"].tolist() == [3, 5] and right["steps"].tolist() == [2, 1] and right["pair_steps"].tolist() == [6, 1]
        assert right["area2"].tolist() == [23_999_999_940, 0] and right["flags"] == ehh_ref.EDGE0
        assert got.pairs[0, 1].tolist() == [[3, 3], [1, 0]]
        got = dev.ehh_scan(dm, g, [0], positions=positions, min_ehh=(11, 100), max_extent=2)
        assert_equal(got, ehh_ref.scan(x, None, mask, [0], positions=positions, min_ehh=(11, 100), max_extent=2), "11/100")
        assert got.sides[0, 1]["steps"].tolist() == [2, 0]
        g.close()
    finally:
        dm.close()


def test_crafted_focal_rows_min_core_and_max_gap(dev):
    rows, cols = 200, 65
    x, called, _ = mosaic_cohort(rows, cols, "multi3-missing", seed=6, switch=0.01, mutation=0.002)
    x, called = x.copy(), called.copy()
    x[50], called[50] = 0, True               # monomorphic: core 1 is empty
    x[60], called[60] = 0, True
    x[60, 17] = 1                             # a singleton core: P_1(0) = 0
    x[70, :6], called[70, 6:12] = 2, False    # members of neither core at the focal row
    called[100] = True
    carriers = np.nonzero(x[100] == 1)[0]     # core 1 of row 100 ends within seven rows (they spell the carrier's index), core 0 walks on
    x[101:108, carriers] = (np.arange(carriers.size)[None, :] >> np.arange(7)[:, None]) & 1
    called[101:108, carriers] = True
    positions = (10 * np.arange(rows)).astype(np.uint32)
    positions[116:] += 100_000                # one gap of 100 010 between rows 115 and 116
    mask = np.ones(cols, dtype=bool)
    focal = [50, 60, 70, 100, 9, 120, 140]
    dm = upload(dev, x, called, 3, planes=True)
    try:
        sides = check(dev, dm, x, called, mask, focal, "crafted", positions=positions, min_ehh=(1, 20), max_gap=50_000)
        assert sides["core"][0, 0].tolist() == [cols, 0] and sides["core"][1, 0].tolist() == [cols - 1, 1]
        assert (sides["steps"][:2, :, 1] == 0).all() and (sides["steps"][:2, :, 0] > 0).all()
        assert sides["core"][2, 0].sum() <= cols - 12 and sides["core"][4, 0].tolist() == [0, 0]  # row 9 is not called at all
        gap_hit = sides["flags"] & GAPS
        assert gap_hit[3, 1] == ehh_ref.GAP0 and 0 < sides["steps"][3, 1, 1] <= 7 and sides["steps"][3, 1, 0] == 15, "max_gap met core 0 after core 1 had ended"
        assert (gap_hit == GAPS).any(), "and both cores at once"
        skipped = check(dev, dm, x, called, mask, focal, "min_core", positions=positions, min_ehh=(1, 20), max_gap=50_000, min_core=2, max_extent=40, curve=True)
        assert (skipped["flags"][[0, 1, 4]] == ehh_ref.SKIPPED).all() and not (skipped["flags"][[2, 3]] & ehh_ref.SKIPPED).any()
        assert not skipped["area2"][[0, 1, 4]].any() and skipped["core"][1, 1].tolist() == [cols - 1, 1]
    finally:
        dm.close()


# ---- long walks, the curve, the grid, streams -------------------------------------------------------------------------------------------
def test_a_mosaic_whose_extents_pass_200_rows(dev):
    x, mask, sides, capped, pairs = prototype_mosaic()
    assert sides["steps"].max() > 200 and np.median(sides["steps"].max(axis=(1, 2))) > 40
    dm = upload(dev, x, None, 1, planes=True)
    try:
        assert_equal(run(dev, dm, mask, PROTOTYPE_FOCAL, min_ehh=(1, 20)), (sides, None), "every third focal row")
        got = run(dev, dm, mask, PROTOTYPE_CURVE_FOCAL, min_ehh=(1, 20), max_extent=230, curve=True, fill=0xEE)  # the buffers start full of junk
        assert_equal(got, (capped, pairs), "curve")
        assert (pairs != 0).sum(axis=3).max() > 200 and (pairs == 0).any()
    finally:
        dm.close()


def test_3000_items_on_seven_workgroups_repeated_and_unordered(dev, fmh_opts):
    x, mask, sides, _, _ = prototype_mosaic()
    which = np.random.default_rng(12).integers(0, len(PROTOTYPE_FOCAL), size=1500)  # repeats, no order
    focal = np.array(PROTOTYPE_FOCAL)[which]
    assert len(set(focal.tolist())) < 1500 and (np.diff(focal) < 0).any()
    dm = upload(dev, x, None, 1, planes=True)
    try:
        fmh_opts.setenv("FMH_GRID_BLOCKS", 7)
        assert_equal(run(dev, dm, mask, focal, min_ehh=(1, 20)), (sides[which], None), "seven workgroups")
    finally:
        dm.close()


@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", ["multi3-missing", "multi7"])
def test_threads_and_grid_change_nothing(dev, fmh_opts, kind, row_hi):
    from ferromic_amd import _abi

    rows, cols = 150, 513
    x, called, positions = mosaic_cohort(rows, cols, kind, seed=13)
    mask = np.random.default_rng(13).random(cols) < 0.5  # about 256 members: four per thread at 64 threads, none for most threads at 1 024
    focal = list(range(0, rows, 5))
    ref = ehh_ref.scan(x, called, mask, focal, positions=positions, min_ehh=(1, 20), max_extent=60, curve=True)
    # rows the tables tell apart, from the cohort itself: with and without an uncalled entry, with and without an allele above 1
    if called is not None:
        assert 0 < int((~called).any(axis=1).sum()) < rows
    assert 0 < int((x > 1).any(axis=1).sum()) < rows
    fmh_opts.setenv("FMH_ROW_HI", row_hi)  # read when the matrix is made: 2 = the row tables at any size, 0 = none
    assert _abi.get_option("FMH_ROW_HI") == int(row_hi)
    dm = upload(dev, x, called, KINDS[kind][0], planes=True)
    try:
        for threads in (None,) + dev.HAP_THREADS:
            if threads is not None:
                fmh_opts.setenv("FMH_HAP_THREADS", threads)
            for per_cu in (None, 1):
                if per_cu is not None:
                    fmh_opts.setenv("FMH_GRID_PER_CU", per_cu)
                else:
                    fmh_opts.delenv("FMH_GRID_PER_CU")
                assert_equal(run(dev, dm, mask, focal, positions=positions, min_ehh=(1, 20), max_extent=60, curve=True), ref, (kind, row_hi, threads, per_cu))
    finally:
        dm.close()


def test_row_tables_by_default_from_4096_rows(dev):
    """A matrix of 4 200 rows gets the row tables without any option.  Focal rows at both ends, next to the all-uncalled row 9 and in the
    middle, both directions; the oracle walks the rows around them only."""
    rows, cols = 4200, 65
    x, called, positions = mosaic_cohort(rows, cols, "multi3-missing", seed=21)
    assert 0 < int((~called).any(axis=1).sum()) < rows and 0 < int((x > 1).any(axis=1).sum()) < rows
    mask = np.ones(cols, dtype=bool)
    focal = [0, 8, 10, 2100, 2101, 4150, rows - 1]
    dm = upload(dev, x, called, 3, planes=True)
    try:
        sides = check(dev, dm, x, called, mask, focal, "default tables", positions=positions, min_ehh=(1, 20))
        check(dev, dm, x, called, mask, focal, "default tables, curve", max_extent=50, curve=True)
        assert sides["steps"].max() > 30 and (sides["flags"] & EDGES).any()
    finally:
        dm.close()


def test_on_a_stream_into_outputs_full_of_junk(dev):
    """The C call on a stream of the caller's, twice, into buffers filled with 0xFF bytes: every entry is written."""
    import torch

    from ferromic_amd import _abi

    lib = _abi.load()
    x, mask, _, capped, pairs = prototype_mosaic()
    focal = np.array(PROTOTYPE_CURVE_FOCAL, dtype=np.uint64)
    params = _abi.EhhParams(1, 20, 230, 0, 0, 0)
    dm = upload(dev, x, None, 1, planes=True)
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        d_out = dev.DeviceBuffer.from_numpy(dm.device, np.full(56 * 2 * focal.size, 0xFF, dtype=np.uint8))
        d_pairs = dev.DeviceBuffer.from_numpy(dm.device, np.full(4 * pairs.size, 0xFF, dtype=np.uint8))
        for call in ("first", "second"):
            _abi.check(lib.fmh_ehh_scan(dm._h, g._h, 0, 400, focal.ctypes.data_as(C.c_void_p), focal.size, None, C.byref(params), d_out.ptr, d_pairs.ptr, handle))
            rec = d_out.to_numpy(np.uint8, 56 * 2 * focal.size).view(dev.EHH_SIDE_DTYPE).reshape(focal.size, 2)
            for field in FIELDS:
                assert np.array_equal(rec[field], capped[field]), (call, field)
            assert np.array_equal(d_pairs.to_numpy(np.uint32, pairs.size).reshape(pairs.shape), pairs), call
    finally:
        stream.synchronize()
        g.close()
        dm.close()


# ---- refusals on a live matrix ----------------------------------------------------------------------------------------------------------
def test_refusals_and_their_order(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, _, _ = mosaic_cohort(17, 513, "complete")
    everyone = np.ones((1, 513), dtype=np.uint8)
    dm = upload(dev, x, None, 1, planes=True)
    other = upload(dev, mosaic_cohort(17, 65, "complete")[0], None, 1, planes=True)
    g = dev.Groups(dm, everyone)
    two = dev.Groups(dm, np.concatenate([everyone, everyone]))
    nobody = dev.Groups(dm, np.zeros((1, 513), dtype=np.uint8))
    foreign = dev.Groups(other, np.ones((1, 65), dtype=np.uint8))
    descending = np.arange(17, dtype=np.uint32) * 5
    descending[8] = 3
    try:
        def refused(call, status, text):
            with pytest.raises(_abi.FerromicHipError) as err:
                call()
            assert err.value.status == status and text in str(err.value), str(err.value)

        bad = _abi.FMH_ERR_INVALID
        refused(lambda: dev.ehh_scan(dm, two, [3]), bad, "exactly 1 group")
        refused(lambda: dev.ehh_scan(dm, foreign, [3]), bad, "not made for this matrix")
        refused(lambda: dev.ehh_scan(dm, nobody, [3]), bad, "no member")
        refused(lambda: dev.ehh_scan(dm, g, [3], row_begin=2, row_end=18), bad, "exceed")
        refused(lambda: dev.ehh_scan(dm, g, [3], row_begin=9, row_end=3), bad, "exceed")
        refused(lambda: dev.ehh_scan(dm, g, [3, 12], row_begin=2, row_end=12), bad, "focal row 12")
        refused(lambda: dev.ehh_scan(dm, g, [1], row_begin=2, row_end=12), bad, "focal row 1")
        refused(lambda: dev.ehh_scan(dm, g, []), bad, "n_focal")
        refused(lambda: dev.ehh_scan(dm, g, [3], min_ehh=(0, 0)), bad, "min_ehh_den")
        refused(lambda: dev.ehh_scan(dm, g, [3], min_ehh=(3, 2)), bad, "min_ehh_num")
        refused(lambda: dev.ehh_scan(dm, g, [3], positions=descending), bad, "descend")
        refused(lambda: dev.ehh_scan(dm, g, [3], curve=True), bad, "max_extent")
        # positions that descend outside the range are nobody's business
        assert_equal(dev.ehh_scan(dm, g, [3], row_begin=0, row_end=8, positions=descending),
                     ehh_ref.scan(x, None, everyone[0], [3], 0, 8, positions=descending), "descent outside the range")
        # the order: each refusal is found before those listed after it
        refused(lambda: dev.ehh_scan(dm, two, [99], row_begin=9, row_end=3), bad, "exactly 1 group")
        refused(lambda: dev.ehh_scan(dm, g, [99], row_begin=9, row_end=3, min_ehh=(0, 0)), bad, "exceed")
        refused(lambda: dev.ehh_scan(dm, g, [99], min_ehh=(0, 0)), bad, "focal row 99")
        refused(lambda: dev.ehh_scan(dm, g, [], min_ehh=(0, 0)), bad, "n_focal")
        refused(lambda: dev.ehh_scan(dm, g, [3], min_ehh=(0, 0), positions=descending), bad, "min_ehh_den")
        refused(lambda: dev.ehh_scan(dm, g, [3], min_ehh=(3, 2), positions=descending), bad, "min_ehh_num")
        refused(lambda: dev.ehh_scan(dm, g, [3], positions=descending, curve=True), bad, "descend")
        # a curve above 2^32 entries: refused before anything of that size exists
        focal = np.zeros(((1 << 32) // 4 // 1000) + 1, dtype=np.uint64)
        params = _abi.EhhParams(0, 1, 1000, 0, 0, 0)
        small = dev.DeviceBuffer(dm.device, 64)
        status = lib.fmh_ehh_scan(dm._h, g._h, 0, 17, focal.ctypes.data_as(C.c_void_p), focal.size, None, C.byref(params), small.ptr, small.ptr, None)
        assert status == _abi.FMH_ERR_UNSUPPORTED and b"2^32" in lib.fmh_last_error()
    finally:
        for h in (g, two, nobody, foreign, dm, other):
            h.close()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    dm = upload(dev, x, None, 1)
    g = dev.Groups(dm, everyone)
    try:
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.ehh_scan(dm, g, [3])
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and "fmh_matrix_pack" in str(err.value)
        dm.pack()
        assert_equal(dev.ehh_scan(dm, g, [3, 0]), ehh_ref.scan(x, None, everyone[0], [3, 0]), "after fmh_matrix_pack")
    finally:
        g.close()
        dm.close()


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------
def python_cohort():
    """80 sites x 12 diploid samples as variant records: a mosaic; site 5 carries an allele 2, site 9 has a sample without a genotype."""
    sites, samples = 80, 12
    x = ehh_ref.mosaic(sites, samples * 2, founders=4, switch=0.03, mutation=0.01, seed=77).copy()
    x[5, 3] = 2
    called = np.ones(x.shape, dtype=bool)
    called[9, 4:6] = False
    positions = 100 + np.cumsum(np.random.default_rng(78).integers(1, 40, size=sites))
    records = []
    for i in range(sites):
        genotypes = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(samples)]
        records.append(dict(position=int(positions[i]), genotypes=genotypes))
    return x, called, positions, records


def assert_python_equal(got, ref_sides, ref_pairs, n, focal, include_edges):
    from tests.test_ehh_cpu import assert_stats_equal

    assert got.sample_size == n and len(got) == len(focal) and got.focal_rows.tolist() == list(focal)
    assert np.array_equal(got.core_counts, ref_sides["core"][:, 0]) and np.array_equal(got.flags, ref_sides["flags"])
    for name in ("area2", "pair_steps", "steps"):
        assert getattr(got, name).shape == (len(focal), 2, 2) and np.array_equal(getattr(got, name), ref_sides[name]), name
    if ref_pairs is None:
        assert got.pairs is None
    else:
        assert np.array_equal(got.pairs, ref_pairs)
    ref = ehh_ref.stats(ref_sides, include_edges)
    assert_stats_equal(dict(ihh=got.ihh, sl=got.sl, ihs=got.ihs, nsl=got.nsl), ref, "python")
    return ref


def test_python_ihs_nsl_and_ehh_scan_of_variant_records(fm):
    x, called, positions, records = python_cohort()
    every = [(s, side) for s in range(12) for side in (0, 1)]
    haps = [h for h in every if h not in ((1, 0), (4, 1), (7, 0))]
    mask = np.zeros(24, dtype=bool)
    for s, side in haps:
        mask[2 * s + side] = True
    rows = list(range(80))
    # ihs: positions, threshold 0.05, minor core at least ceil(0.05 n) members
    for include_edges in (False, True):
        ref = ehh_ref.scan(x, called, mask, rows, positions=positions, min_ehh=(50_000, 1_000_000), min_core=2)
        stats = assert_python_equal(fm.ihs(records, haps, include_edges=include_edges), ref[0], None, 21, rows, include_edges)
        assert np.isfinite(stats["ihs"]).sum() >= (10 if include_edges else 1) and np.isnan(stats["ihs"]).any()
    # nsl: unit distance, no threshold, 100 rows, edges kept
    ref = ehh_ref.scan(x, called, np.ones(24, dtype=bool), rows, max_extent=100)
    stats = assert_python_equal(fm.nsl(records, every), ref[0], None, 24, rows, True)
    assert np.isfinite(stats["nsl"]).sum() > 30
    ref = ehh_ref.scan(x, called, mask, [7, 3, 7], max_extent=5)
    assert_python_equal(fm.nsl(records, haps, focal=[7, 3, 7], max_extent=5), ref[0], None, 21, [7, 3, 7], True)
    # ehh_scan: the caller's parameters; region = rows 20..59, focal rows count inside it
    lo, hi = int(positions[20]), int(positions[59])
    focal = [0, 39, 17, 17]
    ref = ehh_ref.scan(x[20:60], called[20:60], mask, focal, positions=positions[20:60], min_ehh=(250_000, 1_000_000), max_extent=12, max_gap=35, min_core=5, curve=True)
    got = fm.ehh_scan(records, haps, region=(lo, hi), focal=focal, min_ehh=0.25, max_extent=12, max_gap=35, min_maf=0.2, curve=True)
    assert_python_equal(got, ref[0], ref[1], 21, focal, False)
    ref = ehh_ref.scan(x, called, mask, rows, min_ehh=(50_000, 1_000_000))
    assert_python_equal(fm.ehh_scan(records, haps, unit_distance=True, include_edges=True), ref[0], None, 21, rows, True)
    assert "focal=80" in repr(fm.ehh_scan(records, haps))


def test_python_population_scans(fm):
    x, called, positions, records = python_cohort()
    dense = np.where(called, x, -1).astype(np.int8).reshape(80, 12, 2)
    h1 = [(s, side) for s in range(0, 7) for side in (0, 1)]
    h2 = [(s, side) for s in range(5, 12) for side in (0, 1)][1:]
    m1, m2 = np.zeros(24, dtype=bool), np.zeros(24, dtype=bool)
    for s, side in h1:
        m1[2 * s + side] = True
    for s, side in h2:
        m2[2 * s + side] = True
    rows = list(range(80))
    for make in (lambda h: fm.Population.from_numpy("d", dense, positions.astype(np.int64), h, 10_000), lambda h: fm.Population("s", records, h, 10_000)):
        base = make(h1 + h2)
        p1, p2 = base.with_haplotypes(0, h1), base.with_haplotypes(1, h2)
        ref = ehh_ref.scan(x, called, m1, rows, positions=positions, min_ehh=(50_000, 1_000_000), min_core=1)
        assert_python_equal(p1.ihs(), ref[0], None, 14, rows, False)
        ref = ehh_ref.scan(x, called, m2, rows, max_extent=100)
        assert_python_equal(p2.nsl(), ref[0], None, 13, rows, True)
        ref = ehh_ref.scan(x, called, m2, [40, 2], positions=positions, min_ehh=(100_000, 1_000_000), max_extent=9, curve=True)
        assert_python_equal(p2.ehh_scan(focal=[40, 2], min_ehh=0.1, max_extent=9, curve=True), ref[0], ref[1], 13, [40, 2], False)
