"""fmh_sfs / fmh_sfs_joint where tests/test_gpu_sfs.py stops short: a workgroup that takes several work items, rows of more than sixteen
vectors with flaws, and the host paths a caller takes.  Oracle and comparisons as there: tests/sfs_ref.py, array_equal on integers.

A, B  More items than the persistent grid has workgroups (it is min(items, CUs x per_cu), per_cu = 8 for a small tile and 1 for a tile above
      80 KiB), at one row per item: the tile clear in the flush, the reset of the two tallies, the barrier after the flush and the per-item
      table slice run a second and a third time.  The CU count is read from the device and the item count asserted against it.
C     300 x 4 500, a group in vectors 5 .. 34: sixteen lanes, lanes 0 .. 13 take two passes and lanes 14, 15 one, the window starts at
      vector 5.  One-flaw rows for every vector of the window (a single uncalled member, a single allele-2 member) and flaws in non-member
      columns at both ends of the window and just outside it; joint spectra whose union window has a gap neither group covers.
D     70 001 columns: a vector index and a key above 65 535.
E     Every row at one key that goes to the table directly: 6 161 global atomics on one address.
F     9 000 rows with nothing set: three default items, the last partial, windows across the item boundary, row tables by default.
G     The C call on a stream of the caller's into a table filled with 0xFF bytes, twice.

Every case asserts on the oracle alone, before the device is called, that it is not vacuous.

What the file was seen to catch (each change built into a copy of the library and run once on an MI355X; tests/test_gpu_sfs.py stays
green under the first three): no `tile[s] = 0` in the flush - A, B; no `s_skip[tid] = 0` - A on every matrix that has tallies; `out`
taken once from the workgroup's first item - A, B; a single pass over the vectors - B, C, D; the joint window from group 0 alone - the
joint calls of A, C, F, G; no clear of the table - G by construction, and everything else but B and the joint table of D, whose fresh allocations happened to be zero.
"""

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import sfs_ref
from tests.test_gpu_sfs import KINDS, assert_sfs_equal, cohort, group_masks, members, run_joint, run_sfs, upload

pytestmark = pytest.mark.gpu

GRID_ROWS, GRID_COLS = 6161, 257
BINS = ["4", None]
BINS_IDS = ["bins=4", "bins=default"]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def set_option(fmh_opts, key, value):
    if value is None:
        fmh_opts.delenv(key)
    else:
        fmh_opts.setenv(key, value)


def near_edge(n, bins):
    """The keys 0 .. n of an axis that a tile of `bins` slots keeps on chip (all of them when the axis fits)."""
    k = np.arange(n + 1)
    return np.ones(n + 1, dtype=bool) if n + 1 <= bins else np.minimum(k, n - k) < bins // 2


def assert_joint_equal(got, ref, what):
    assert got.counts.dtype == np.uint64 and got.counts.shape == ref[0].shape, what
    assert np.array_equal(got.counts, ref[0]), what
    assert (got.multiallelic, got.incomplete) == ref[1:], what


def assert_flawed_kind(ref_multi, ref_incomplete, max_allele, missing):
    assert (ref_multi > 0) == (max_allele > 1) and (ref_incomplete > 0) == missing


# ---- A: several items per workgroup, 256 threads --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case(kind):
    max_allele, missing = KINDS[kind]
    x, called = cohort(GRID_ROWS, GRID_COLS, max_allele, missing)
    masks = group_masks(GRID_COLS, 3)
    half, last = masks["half"], masks["last-vector"]
    one_row = [(r, r + 1) for r in range(GRID_ROWS)]
    whole = sfs_ref.sfs(x, called, half, [(0, GRID_ROWS)])
    k, multi, incomplete = sfs_ref.classify(x, called, half)
    return SimpleNamespace(x=x, called=called, max_allele=max_allele, missing=missing, half=half, last=last, n=int(half.sum()), whole=whole,
                           one_row_windows=one_row, one_row=sfs_ref.sfs(x, called, half, one_row), k=k, usable=~multi & ~incomplete,
                           joint=sfs_ref.sfs_joint(x, called, half, last, 0, GRID_ROWS))


@pytest.mark.parametrize("bins", BINS, ids=BINS_IDS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_workgroup_takes_three_items(dev, fmh_opts, cus, kind, bins):
    co = grid_case(kind)
    n = co.n
    # not vacuous: one row per item and more than three items for each of the 8 x CUs workgroups of a small tile
    assert GRID_ROWS > 3 * 8 * cus, f"{cus} CUs: {GRID_ROWS} one-row items no longer give every workgroup three"
    assert 100 < n < 160 and int(co.whole[0][0].sum()) > 300 and len(np.nonzero(co.whole[0][0][1:n])[0]) >= 24
    assert_flawed_kind(co.whole[1][0], co.whole[2][0], co.max_allele, co.missing)
    if bins is not None:
        inside = near_edge(n, int(bins))
        on_chip = int(co.whole[0][0][inside].sum())
        assert on_chip * 5 > int(co.whole[0][0].sum()) and co.whole[0][0][~inside].any(), "tile keys and direct keys are both occupied"
        # consecutive items of ONE workgroup (stride = the grid) are tile keys again and again: a bin left behind would be added twice
        tile_rows = co.usable & inside[np.minimum(co.k, n)]
        assert (tile_rows[: GRID_ROWS - 8 * cus] & tile_rows[8 * cus:]).sum() > 50
    fmh_opts.setenv("FMH_SFS_ITEM_ROWS", "1")
    set_option(fmh_opts, "FMH_SFS_LDS_BINS", bins)
    dm = upload(dev, co.x, co.called, co.max_allele, planes=co.missing)
    try:
        assert_sfs_equal(run_sfs(dev, dm, co.half, [(0, GRID_ROWS)]), co.whole, (kind, bins, "one window"))
        got = run_sfs(dev, dm, co.half, co.one_row_windows)
        assert_sfs_equal(got, co.one_row, (kind, bins, "one-row windows"))
        assert np.array_equal(got.counts.sum(axis=1) + got.multiallelic + got.incomplete, np.ones(GRID_ROWS, dtype=np.uint64))
        assert np.array_equal(got.counts.sum(axis=0), co.whole[0][0])
        assert_joint_equal(run_joint(dev, dm, co.half, co.last), co.joint, (kind, bins, "joint"))
    finally:
        dm.close()


# ---- B: several items per workgroup, 512 threads --------------------------------------------------------------------------------------
def test_every_wide_workgroup_takes_two_items(dev, fmh_opts, cus):
    """600 rows x 20 600 columns, everyone a member, the largest tile: 20 601 bins are 82 420 bytes with the head, more than half a CU's LDS,
    so one 512-thread workgroup per CU walks 600 one-row items."""
    rows, n = 600, 20600
    assert rows > 2 * cus, f"{cus} CUs: {rows} one-row items no longer give every workgroup two"
    assert n + 1 <= dev.SFS_MAX_LDS_BINS and (n + 1 + 4) * 4 > (160 << 10) // 2
    x = cohort(rows, n, 1, False)[0].copy()
    rng = np.random.default_rng(20600)
    crafted = (0, 1, n - 1, n, n // 2, n // 2, n // 2 + 1, 0, n, 1, n - 1, n // 2 - 1)
    at = rng.choice(np.arange(6, rows), size=len(crafted), replace=False)
    for r, k in zip(at, crafted):
        x[r] = 0
        x[r, rng.choice(n, size=k, replace=False)] = 1
    mask = np.ones(n, dtype=bool)
    ref = sfs_ref.sfs(x, None, mask, [(0, rows)])
    assert ref[0][0][[0, 1, n - 1, n]].min() >= 2 and ref[0][0][n // 2] == 2 and len(np.nonzero(ref[0][0][1:n])[0]) >= 50
    # the same key from two items of one workgroup (rows a grid apart): the second flush must not see the first one's bin
    k = x.sum(axis=1)
    assert len(np.unique(k)) < rows and ref[0][0].max() >= 3
    fmh_opts.setenv("FMH_SFS_LDS_BINS", str(dev.SFS_MAX_LDS_BINS))
    fmh_opts.setenv("FMH_SFS_ITEM_ROWS", "1")
    dm = upload(dev, x, None, 1)
    try:
        got = run_sfs(dev, dm, mask, [(0, rows)])
        assert_sfs_equal(got, ref, "512 threads, one row per item")
        got = run_sfs(dev, dm, mask, [(r, r + 1) for r in range(rows)])
        assert_sfs_equal(got, sfs_ref.sfs(x, None, mask, [(r, r + 1) for r in range(rows)]), "512 threads, one-row windows")
    finally:
        dm.close()


# ---- C: wide rows with flaws, sixteen lanes, offset window ------------------------------------------------------------------------------
WIDE_ROWS, WIDE_COLS = 300, 4500
WIDE_FIRST, WIDE_LAST = 5, 34  # the vectors of the group
OUTSIDE = {"vector 5": 640, "vector 34": 4450, "vector 4": 600, "vector 35": 4490}  # non-member columns


def vector_range(mask):
    at = np.nonzero(mask)[0]
    return int(at[0]) // 128, int(at[-1]) // 128


@functools.lru_cache(maxsize=None)
def wide_groups():
    rng = np.random.default_rng(4500)
    wide = np.zeros(WIDE_COLS, dtype=bool)
    wide[641:4401] = rng.random(4401 - 641) < 0.6
    wide[641] = wide[4400] = True
    low = np.zeros(WIDE_COLS, dtype=bool)  # vectors 0 .. 2
    low[:384] = rng.random(384) < 0.6
    low[0] = low[383] = True
    end = np.zeros(WIDE_COLS, dtype=bool)
    end[WIDE_COLS - 1] = True
    return wide, low, end


@functools.lru_cache(maxsize=None)
def wide_case(kind):
    """The 300 x 4 500 cohort of the kind with one-flaw rows written over some of its rows; marks[(flaw, place)] = the row."""
    max_allele, missing = KINDS[kind]
    x, called = cohort(WIDE_ROWS, WIDE_COLS, max_allele, missing)
    x = x.copy()
    called = None if called is None else called.copy()
    wide, low, end = wide_groups()
    rng = np.random.default_rng(4501)
    free = [int(r) for r in rng.permutation(WIDE_ROWS) if r > 5]
    flaws = (["uncalled"] if missing else []) + (["high"] if max_allele > 1 else [])
    marks = {}

    def one_flaw(flaw, place, column):
        r = free.pop()
        marks[(flaw, place)] = r
        x[r] &= 1
        if called is not None:
            called[r] = True
        if flaw == "uncalled":
            x[r, column] = 1
            called[r, column] = False
        else:
            x[r, column] = 2

    for v in range(WIDE_FIRST, WIDE_LAST + 1):
        inside = np.nonzero(wide[v * 128:(v + 1) * 128])[0] + v * 128
        for flaw in flaws:
            one_flaw(flaw, v, int(inside[0] if v % 2 else inside[-1]))  # the first or the last member of the vector
    for place, column in OUTSIDE.items():
        for flaw in flaws:
            one_flaw(flaw, place, column)
    for a in (x, called):
        if a is not None:
            a.setflags(write=False)
    return SimpleNamespace(x=x, called=called, max_allele=max_allele, missing=missing, flaws=flaws, marks=marks)


def assert_wide_not_vacuous(co, wide, low, end):
    assert vector_range(wide) == (WIDE_FIRST, WIDE_LAST) and vector_range(low) == (0, 2) and vector_range(end) == (35, 35)
    # 30 vectors over sixteen lanes: lanes 0 .. 13 read two, lanes 14 and 15 one
    assert WIDE_LAST + 1 - WIDE_FIRST == 30 and not (wide | low)[3 * 128:5 * 128].any()
    assert OUTSIDE["vector 5"] // 128 == 5 and OUTSIDE["vector 34"] // 128 == 34 and OUTSIDE["vector 4"] // 128 == 4 and OUTSIDE["vector 35"] // 128 == 35
    assert not any(wide[c] or low[c] or end[c] for c in OUTSIDE.values())
    k, multi, incomplete = sfs_ref.classify(co.x, co.called, wide)
    everyone_called = np.ones(co.x.shape, dtype=bool) if co.called is None else co.called
    for (flaw, place), r in co.marks.items():
        uncalled, high = np.nonzero(~everyone_called[r])[0], np.nonzero(co.x[r] > 1)[0]
        at = uncalled if flaw == "uncalled" else high
        assert at.size == 1 and uncalled.size + high.size == 1, (flaw, place)
        if place in OUTSIDE:
            assert at[0] == OUTSIDE[place] and not multi[r] and not incomplete[r], (flaw, place)
        else:
            assert at[0] // 128 == place and wide[at[0]] and (incomplete[r] if flaw == "uncalled" else multi[r]), (flaw, place)
    assert len(co.marks) == 34 * len(co.flaws)
    assert int((~multi & ~incomplete).sum()) > 100


@pytest.mark.parametrize("row_hi", ["0", "2", None], ids=["row_hi=0", "row_hi=2", "row_hi=default"])
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_thirty_vectors_from_vector_five_with_one_flaw_rows(dev, fmh_opts, kind, planes, row_hi):
    co = wide_case(kind)
    wide, low, end = wide_groups()
    assert_wide_not_vacuous(co, wide, low, end)
    n = int(wide.sum())
    windows = [(0, WIDE_ROWS), (137, WIDE_ROWS)]
    ref = sfs_ref.sfs(co.x, co.called, wide, windows)
    assert len(np.nonzero(ref[0][1][1:n])[0]) >= 24
    assert_flawed_kind(ref[1][1], ref[2][1], co.max_allele, co.missing)
    marked = sorted(co.marks.items(), key=lambda item: item[1])
    set_option(fmh_opts, "FMH_ROW_HI", row_hi)
    dm = upload(dev, co.x, co.called, co.max_allele, planes)
    try:
        assert_sfs_equal(run_sfs(dev, dm, wide, windows), ref, (kind, planes, row_hi))
        if marked:  # per row: a window of its own for every marked row
            rows_of = [(r, r + 1) for _, r in marked]
            got = run_sfs(dev, dm, wide, rows_of)
            assert_sfs_equal(got, sfs_ref.sfs(co.x, co.called, wide, rows_of), (kind, planes, row_hi, "marked rows"))
            for w, ((flaw, place), r) in enumerate(marked):
                tally = (int(got.counts[w].sum()), int(got.multiallelic[w]), int(got.incomplete[w]))
                want = (1, 0, 0) if place in OUTSIDE else (0, 0, 1) if flaw == "uncalled" else (0, 1, 0)
                assert tally == want, (kind, planes, row_hi, flaw, place, r, tally)
        # joint: the union window is vectors 0 .. 34 with vectors 3 and 4 in neither mask (both orders), and vectors 5 .. 35
        for a, b, what in ((wide, low, "wide x low"), (low, wide, "low x wide"), (wide, end, "wide x last column")):
            ref_joint = sfs_ref.sfs_joint(co.x, co.called, a, b, 0, WIDE_ROWS)
            assert int(ref_joint[0].sum()) > 100
            assert_joint_equal(run_joint(dev, dm, a, b), ref_joint, (kind, planes, row_hi, what))
        ref_joint = sfs_ref.sfs_joint(co.x, co.called, wide, low, 137, 163)
        assert_joint_equal(run_joint(dev, dm, wide, low, 137, 163), ref_joint, (kind, planes, row_hi, "rows 137 .. 299"))
    finally:
        dm.close()


# ---- D: more than 65 535 columns --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case():
    rows, cols = 40, 70001
    x, called = cohort(rows, cols, 3, True)
    x, called = x.copy(), called.copy()
    rng = np.random.default_rng(70001)
    tail = np.zeros(cols, dtype=bool)
    tail[65000:70001] = rng.random(5001) < 0.5
    tail[70000] = True
    # clean rows at both ends of the axis of 70 001 (at 64 bins the tile holds k < 32 and n - k < 32) and in the middle
    for r, k in zip(range(8, 20), (0, 1, 31, 32, cols - 32, cols - 31, cols - 1, cols, 33000, 40000, 31, cols - 31)):
        x[r] = 0
        x[r, rng.choice(cols, size=k, replace=False)] = 1
        called[r] = True
    for a in (x, called):
        a.setflags(write=False)
    return x, called, np.ones(cols, dtype=bool), tail


@pytest.mark.parametrize("bins", ["64", None], ids=["bins=64", "bins=default"])
def test_more_than_65535_columns(dev, fmh_opts, bins):
    x, called, everyone, tail = long_case()
    rows, cols = x.shape
    budget = dev.SFS_DEFAULT_LDS_BINS if bins is None else int(bins)
    windows = [(0, rows), (7, 31)]
    refs = {}
    for name, mask in (("all", everyone), ("tail", tail)):
        n = int(mask.sum())
        refs[name] = ref = sfs_ref.sfs(x, called, mask, windows)
        assert ref[1][0] > 0 and ref[2][0] > 0 and ref[0][0].sum() >= 12
        inside = near_edge(n, budget)
        assert ref[0][0][inside].any() and (inside.all() or ref[0][0][~inside].any()), (name, "tile keys and direct keys")
    assert cols > 65535 and vector_range(tail)[0] > 500 and np.nonzero(refs["all"][0][0])[0].max() == cols
    assert not near_edge(cols, budget).all() and (bins is None or not near_edge(int(tail.sum()), budget).all())
    set_option(fmh_opts, "FMH_SFS_LDS_BINS", bins)
    dm = upload(dev, x, called, 3, planes=True)
    try:
        for name, mask in (("all", everyone), ("tail", tail)):
            assert_sfs_equal(run_sfs(dev, dm, mask, windows), refs[name], (bins, name))
    finally:
        dm.close()


def test_joint_of_70001_and_2538_members(dev, fmh_opts):
    """The widest table the suite asks for: 70 002 x 2 539 bins (1.4 GB of u64, within the 2^28-bin limit), corners of 4 x 4 keys on chip."""
    x, called, everyone, tail = long_case()
    rows, cols = x.shape
    n1 = int(tail.sum())
    assert (cols + 1) * (n1 + 1) <= 1 << 28
    ref = sfs_ref.sfs_joint(x, called, everyone, tail, 0, rows)
    assert ref[1] > 0 and ref[2] > 0
    corner = near_edge(cols, 8)[:, None] & near_edge(n1, 8)[None, [0, 1, 2, 3, n1 - 3, n1 - 2, n1 - 1, n1]]
    on_chip = int(ref[0][:, [0, 1, 2, 3, n1 - 3, n1 - 2, n1 - 1, n1]][corner].sum())
    assert 0 < on_chip < int(ref[0].sum())
    fmh_opts.setenv("FMH_SFS_LDS_BINS", "64")
    dm = upload(dev, x, called, 3, planes=True)
    try:
        assert_joint_equal(run_joint(dev, dm, everyone, tail), ref, "70 001 x tail")
    finally:
        dm.close()


# ---- E: one contended address -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_rows", ["1", None], ids=["item=1", "item=default"])
def test_every_row_adds_to_one_bin_of_the_table(dev, fmh_opts, item_rows):
    x = cohort(GRID_ROWS, GRID_COLS, 1, False)[0].copy()
    mask = group_masks(GRID_COLS, 3)["half"]
    at = np.nonzero(mask)[0]
    n = at.size
    rng = np.random.default_rng(6161)
    for r in range(GRID_ROWS):
        x[r, at] = 0
        x[r, rng.permutation(at)[: n // 2]] = 1
    ref = sfs_ref.sfs(x, None, mask, [(0, GRID_ROWS)])
    want = np.zeros(n + 1, dtype=np.uint64)
    want[n // 2] = GRID_ROWS
    assert np.array_equal(ref[0][0], want) and not near_edge(n, 4)[n // 2]  # every row goes past the tile
    fmh_opts.setenv("FMH_SFS_LDS_BINS", "4")
    set_option(fmh_opts, "FMH_SFS_ITEM_ROWS", item_rows)
    dm = upload(dev, x, None, 1)
    try:
        got = run_sfs(dev, dm, mask, [(0, GRID_ROWS)])
        assert_sfs_equal(got, ref, item_rows)
        assert got.counts[0][n // 2] == GRID_ROWS and int(got.counts[0].sum()) == GRID_ROWS
    finally:
        dm.close()


# ---- F: default items and tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
def test_default_items_across_their_boundaries(dev, fmh_opts, planes):
    rows, cols = 9000, 257
    assert 2 * dev.SFS_DEFAULT_ITEM_ROWS < rows < 3 * dev.SFS_DEFAULT_ITEM_ROWS
    x, called = cohort(rows, cols, 3, True)
    mask = group_masks(cols, 3)["half"]
    windows = [(0, rows), (4095, 4097), (4096, 8192), (1, rows - 1), (4096, 4096)]
    ref = sfs_ref.sfs(x, called, mask, windows)
    assert ref[1][0] > 0 and ref[2][0] > 0 and ref[0][0].sum() > 300 and ref[0][1].sum() + ref[1][1] + ref[2][1] == 2
    joint = sfs_ref.sfs_joint(x, called, mask, members(cols, 40, 9), 1, rows - 2)
    tables = []
    for row_hi in (None, "0"):  # untouched: 9 000 rows get their row tables
        set_option(fmh_opts, "FMH_ROW_HI", row_hi)
        dm = upload(dev, x, called, 3, planes)
        try:
            got = run_sfs(dev, dm, mask, windows)
            assert_sfs_equal(got, ref, (planes, row_hi))
            widths = np.array([e - b for b, e in windows], dtype=np.uint64)
            assert np.array_equal(got.counts.sum(axis=1) + got.multiallelic + got.incomplete, widths)
            got_joint = run_joint(dev, dm, mask, members(cols, 40, 9), 1, rows - 2)
            assert_joint_equal(got_joint, joint, (planes, row_hi, "joint"))
            tables.append((got.counts, got_joint.counts))
        finally:
            dm.close()
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])


# ---- G: a stream of the caller's and a table that is not zero -----------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BINS, ids=BINS_IDS)
def test_on_a_stream_into_a_table_full_of_ones(dev, fmh_opts, bins):
    import torch

    from ferromic_amd import _abi

    lib = _abi.load()
    rows, cols = 300, 513
    x, called = cohort(rows, cols, 3, True)
    m0, m1 = members(cols, 257, 257), members(cols, 40, 40)
    windows = [(0, rows), (10, 200), (299, 300)]
    w = np.array(windows, dtype=np.uint64)
    ref = sfs_ref.sfs(x, called, m0, windows)
    ref_joint = sfs_ref.sfs_joint(x, called, m0, m1, 7, 250)
    assert ref[1][0] > 0 and ref[2][0] > 0 and ref_joint[1] > 0 and ref_joint[2] > 0
    assert (ref[0] == 0).sum() > 100 and (ref_joint[0] == 0).sum() > 100  # bins nothing is added to: only the clear makes them zero
    set_option(fmh_opts, "FMH_SFS_LDS_BINS", bins)
    dm = upload(dev, x, called, 3, planes=True)
    g1 = dev.Groups(dm, m0[None, :].astype(np.uint8))
    g2 = dev.Groups(dm, np.stack([m0, m1]).astype(np.uint8))
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        d_sfs = dev.DeviceBuffer.from_numpy(dm.device, np.full(ref[0].size * 8, 0xFF, dtype=np.uint8))
        d_joint = dev.DeviceBuffer.from_numpy(dm.device, np.full(ref_joint[0].size * 8, 0xFF, dtype=np.uint8))
        for call in ("first", "second"):  # the second call finds the first one's table
            skipped = (_abi.SfsSkipped * len(windows))()
            _abi.check(lib.fmh_sfs(dm._h, g1._h, w.ctypes.data_as(C.c_void_p), len(windows), d_sfs.ptr, skipped, handle))
            counts = d_sfs.to_numpy(np.uint64, ref[0].size).reshape(ref[0].shape)
            assert np.array_equal(counts, ref[0]), (bins, call)
            assert [int(s.multiallelic) for s in skipped] == ref[1].tolist() and [int(s.incomplete) for s in skipped] == ref[2].tolist()
            skipped = (_abi.SfsSkipped * 1)()
            _abi.check(lib.fmh_sfs_joint(dm._h, g2._h, 7, 250, d_joint.ptr, skipped, handle))
            counts = d_joint.to_numpy(np.uint64, ref_joint[0].size).reshape(ref_joint[0].shape)
            assert np.array_equal(counts, ref_joint[0]), (bins, call, "joint")
            assert (int(skipped[0].multiallelic), int(skipped[0].incomplete)) == ref_joint[1:]
    finally:
        stream.synchronize()
        g1.close()
        g2.close()
        dm.close()
