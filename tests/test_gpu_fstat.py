"""The f-statistics' moment table on the device (fmh_fstat_moments) against tests/fstat_ref.py, the oracle written from the definition.
Every comparison is array_equal on integers: the u64 table and the two tallies, and the same table again under every route (rows per item,
mask entries in LDS or in global memory, row tables on or off, a caller's stream, a table that is not zero beforehand).

Cohorts are those of tests/test_gpu_sfs.py (complete, missing, multi3-missing, multi7; the flaws sit in a third of the rows each, one row is
entirely uncalled, from_host_planes puts junk under the uncalled entries).  Shapes are the smallest at which each part of the kernel can go
wrong: a partial last dword and vector, rows of one to five vectors (four lanes per row up to four vectors, sixteen beyond), row counts
around the 16 and 64 rows of a pass, 300 rows for several passes and items; 2 to 32 groups - 26 and 32 give a thread two and three slots of
the slice (378 and 561 slots over 256 threads), fewer than 256 slots share a pass's rows among thread groups.

Every case with at least 15 rows asserts, on the oracle alone and before the device is called, that some block has a usable row.

Refusal 6 (a block of rows x max(n)^2 >= 2^63) needs 2^45 rows at 513 columns: it is asked of a wrapped matrix that declares them over a
few bytes - the refusal comes before anything reads the matrix, and before refusal 7, which that matrix (u8 rows only) would also earn.
"""

import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import fstat_ref
from tests.test_fstat_cpu import JACKKNIFE_MARGIN, JACKKNIFE_MEASURED
from tests.test_gpu_sfs import KINDS, cohort, python_cohort, upload

pytestmark = pytest.mark.gpu

COLUMNS = [2, 63, 64, 65, 129, 257, 513]
ROWS = [1, 3, 15, 16, 17, 300]
GROUPS = [2, 3, 5, 8, 9, 26, 32]
MEMBERSHIPS = ["partition", "interleaved", "halves", "one-member", "last-vector", "gaps"]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


@pytest.fixture(scope="module")
def cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def set_option(fmh_opts, key, value):
    if value is None:
        fmh_opts.delenv(key)
    else:
        fmh_opts.setenv(key, value)


# ---- memberships ----------------------------------------------------------------------------------------------------------------------
def halves(cols, G, rng):
    masks = rng.random((G, cols)) < 0.5
    for g in range(G):
        masks[g, rng.integers(cols)] = True
    return masks


def membership(name, cols, G, seed=0):
    """G boolean column masks, every group with a member; None where the kind needs more columns than there are."""
    rng = np.random.default_rng(100 * cols + G + seed)
    if name in ("partition", "interleaved"):
        if cols < G:
            return None
        masks = np.zeros((G, cols), dtype=bool)
        if name == "partition":  # contiguous, unequal
            for g, part in enumerate(np.array_split(np.arange(cols), G)):
                masks[g, part] = True
        else:
            masks[np.arange(cols) % G, np.arange(cols)] = True
        return masks
    masks = halves(cols, G, rng)
    if name == "one-member":
        masks[0] = False
        masks[0, cols // 3] = True
    elif name == "last-vector":  # the last group only in the last (partial) 16-byte vector
        first_of_last = (cols - 1) // 128 * 128
        masks[G - 1] = False
        masks[G - 1, first_of_last:] = rng.random(cols - first_of_last) < 0.6
        masks[G - 1, cols - 1] = True
    elif name == "gaps":  # nobody in the odd vectors (where there are any), and a hole of uncovered columns in every vector
        column = np.arange(cols)
        masks[:, (column // 128) % 2 == 1] = False
        masks[:, column % 16 == 5] = False
        for g in range(G):
            if not masks[g].any():
                masks[g, 0] = True
    return masks


def assert_moments_equal(got, ref, what):
    table, multi, incomplete = ref
    assert got.moments.dtype == np.uint64 and got.moments.shape == table.shape, what
    assert np.array_equal(got.moments, table), what
    assert np.array_equal(got.multiallelic, multi) and np.array_equal(got.incomplete, incomplete), what


def geometry_cases(kind):
    """(cols, rows, membership, G, masks, blocks, oracle result) of the geometry test: every column count x row count x membership, the
    group count rotating so that each (columns, G) and each (membership, G) pair comes up."""
    max_allele, missing = KINDS[kind]
    for ci, cols in enumerate(COLUMNS):
        for ri, rows in enumerate(ROWS):
            x, called = cohort(rows, cols, max_allele, missing)
            blocks = [(0, rows), (rows // 2, rows)]
            for mi, name in enumerate(MEMBERSHIPS):
                G = GROUPS[(ci + ri + 2 * mi) % len(GROUPS)]
                masks = membership(name, cols, G)
                if masks is None:  # fewer columns than groups: the smallest group count instead
                    G = 2
                    masks = membership(name, cols, G)
                yield cols, rows, name, G, masks, blocks, fstat_ref.moments(x, called, masks, blocks)


# ---- geometry x matrix kinds x memberships ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_geometry_membership_and_group_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    seen_multi = seen_incomplete = 0
    seen = set()
    matrices = {}
    try:
        for cols, rows, name, G, masks, blocks, ref in geometry_cases(kind):
            if rows >= 15:
                assert ref[0][:, 0].max() > 0, (cols, rows, name, G, "no usable row in any block")
            if (cols, rows) not in matrices:
                for dm in matrices.values():
                    dm.close()
                matrices.clear()
                x, called = cohort(rows, cols, max_allele, missing)
                matrices[(cols, rows)] = upload(dev, x, called, max_allele, planes)
            got = dev.fstat_moments(matrices[(cols, rows)], masks, blocks)
            assert_moments_equal(got, ref, (cols, rows, name, G))
            # every row is accounted for
            assert int(got.moments[0, 0] + got.multiallelic[0] + got.incomplete[0]) == rows
            seen_multi += int(ref[1][0])
            seen_incomplete += int(ref[2][0])
            seen.add((name, G))
            seen.add(("columns", cols, G))
    finally:
        for dm in matrices.values():
            dm.close()
    # not vacuous (from the oracle): the tallies the kind is about, and every group count under every membership
    assert (seen_incomplete > 0) == missing and (seen_multi > 0) == (max_allele > 1)
    assert all((name, G) in seen for name in MEMBERSHIPS for G in GROUPS)
    assert all(("columns", cols, G) in seen for cols in COLUMNS[1:] for G in GROUPS)


# ---- vectors nobody covers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
def test_flaws_count_where_any_group_has_a_member_and_nowhere_else(dev, planes):
    """513 columns = vectors 0 .. 4.  Group 0 in vector 0, group 1 in vectors 0 and 2, group 2 in the one column of vector 4; vectors 1 and 3
    belong to nobody.  Rows with ONE flaw each: in vector 1 or 3, or in a non-member column of vector 0 or 2 - usable; at a member of
    group 1 only, of group 2 only - flagged for all three groups."""
    rows, cols = 40, 513
    x, called = cohort(rows, cols, 1, False, seed=3)
    x = x.copy()
    called = np.ones(x.shape, dtype=bool)
    masks = np.zeros((3, cols), dtype=bool)
    masks[0, 3:100:2] = True
    masks[1, 4:100:2] = True
    masks[1, 256:380:3] = True
    masks[2, 512] = True
    covered = masks.any(axis=0)
    spots = {"vector 1": 130, "vector 3": 500, "hole in vector 0": 101, "hole in vector 2": 257, "group 1 only, vector 2": 256,
             "group 2 only": 512, "group 0 only": 3}
    want = {}
    r = 5
    for flaw in ("uncalled", "high"):
        for place, column in spots.items():
            assert covered[column] == ("only" in place) and (column // 128 == int(place[-1]) if "vector" in place else True)
            if flaw == "uncalled":
                called[r, column] = False
                x[r, column] = 1  # junk under the uncalled entry of the allele plane
            else:
                x[r, column] = 2
            want[r] = (flaw, place)
            r += 1
    ref = fstat_ref.moments(x, called, masks, [(0, rows)] + [(r, r + 1) for r in want])
    for w, (r, (flaw, place)) in enumerate(want.items(), start=1):
        tally = (int(ref[0][w, 0]), int(ref[1][w]), int(ref[2][w]))
        assert tally == ((1, 0, 0) if "only" not in place else (0, 0, 1) if flaw == "uncalled" else (0, 1, 0)), (flaw, place)
    assert ref[0][0, 0] == rows - 6 and ref[1][0] == 3 and ref[2][0] == 3
    dm = upload(dev, x, called, 3, planes)
    try:
        assert_moments_equal(dev.fstat_moments(dm, masks, [(0, rows)] + [(r, r + 1) for r in want]), ref, planes)
    finally:
        dm.close()


# ---- blocks and routes on 300 rows -----------------------------------------------------------------------------------------------------------
BLOCK_SETS = {
    "one": [(0, 300)],
    "unequal": [(0, 1), (1, 18), (18, 82), (82, 83), (83, 300)],
    "overlapping-empty-unordered": [(200, 300), (0, 0), (0, 120), (100, 250), (100, 250), (300, 300), (17, 18), (150, 150)],
}


@functools.lru_cache(maxsize=None)
def route_case(kind, G):
    max_allele, missing = KINDS[kind]
    cols, rows = 257, 300
    x, called = cohort(rows, cols, max_allele, missing, seed=11)
    masks = membership("halves", cols, G, seed=11)
    refs = {name: fstat_ref.moments(x, called, masks, blocks) for name, blocks in BLOCK_SETS.items()}
    return x, called, masks, refs


@pytest.mark.parametrize("G", [9, 32])
@pytest.mark.parametrize("kind", ["missing", "multi3-missing"])
def test_blocks_under_every_route(dev, fmh_opts, kind, G):
    """Rows per item 1, 7 and the default; the mask entries in LDS and forced to global memory; row tables off, forced and by default;
    the NULL stream and a caller's; a fresh table and one full of 0xFF bytes: one and the same table."""
    import torch

    from ferromic_amd import _abi

    lib = _abi.load()
    max_allele, missing = KINDS[kind]
    x, called, masks, refs = route_case(kind, G)
    whole = refs["one"]
    assert whole[0][0, 0] > 50 and whole[2][0] > 0 and (whole[1][0] > 0) == (max_allele > 1)
    width = fstat_ref.moment_count(G)
    masks_u8 = np.ascontiguousarray(masks, dtype=np.uint8)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    tables = []
    try:
        for row_hi in ("0", "2", None):
            set_option(fmh_opts, "FMH_ROW_HI", row_hi)
            dm = upload(dev, x, called, max_allele, planes=True)
            try:
                for item_rows in ("1", "7", None):
                    set_option(fmh_opts, "FMH_FSTAT_ITEM_ROWS", item_rows)
                    for mask_bytes in ("1", None):
                        set_option(fmh_opts, "FMH_FSTAT_LDS_MASK_BYTES", mask_bytes)
                        what = (kind, G, row_hi, item_rows, mask_bytes)
                        for name, blocks in BLOCK_SETS.items():
                            got = dev.fstat_moments(dm, masks, blocks)
                            assert_moments_equal(got, refs[name], what + (name,))
                            widths = np.array([e - b for b, e in blocks], dtype=np.uint64)
                            assert np.array_equal(got.moments[:, 0] + got.multiallelic + got.incomplete, widths), what + (name,)
                        # the C call on a stream of the caller's into a table full of ones, twice (the second finds the first one's table)
                        blocks = np.array(BLOCK_SETS["unequal"], dtype=np.uint64)
                        ref = refs["unequal"]
                        d_table = dev.DeviceBuffer.from_numpy(dm.device, np.full(ref[0].size * 8, 0xFF, dtype=np.uint8))
                        for call in ("first", "second"):
                            skipped = (_abi.SfsSkipped * len(blocks))()
                            _abi.check(lib.fmh_fstat_moments(dm._h, masks_u8.ctypes.data_as(C.c_void_p), G, blocks.ctypes.data_as(C.c_void_p),
                                                             len(blocks), d_table.ptr, skipped, handle))
                            table = d_table.to_numpy(np.uint64, ref[0].size).reshape(len(blocks), width)
                            assert np.array_equal(table, ref[0]), what + (call,)
                            assert [int(s.multiallelic) for s in skipped] == ref[1].tolist() and [int(s.incomplete) for s in skipped] == ref[2].tolist()
                        tables.append(table)
                        # without tallies, and all blocks empty: a zeroed table
                        _abi.check(lib.fmh_fstat_moments(dm._h, masks_u8.ctypes.data_as(C.c_void_p), G, blocks.ctypes.data_as(C.c_void_p), len(blocks),
                                                         d_table.ptr, None, None))
                        assert np.array_equal(d_table.to_numpy(np.uint64, ref[0].size).reshape(len(blocks), width), ref[0]), what
                        empty = np.array([(5, 5), (300, 300)], dtype=np.uint64)
                        _abi.check(lib.fmh_fstat_moments(dm._h, masks_u8.ctypes.data_as(C.c_void_p), G, empty.ctypes.data_as(C.c_void_p), 2, d_table.ptr, None, handle))
                        assert not d_table.to_numpy(np.uint64, 2 * width).any(), what
            finally:
                stream.synchronize()
                dm.close()
    finally:
        stream.synchronize()
    assert len(tables) == 18 and all(np.array_equal(tables[0], t) for t in tables[1:])


# ---- more one-row items than the persistent grid has workgroups ------------------------------------------------------------------------------
GRID_ROWS, GRID_COLS = 6161, 257


@functools.lru_cache(maxsize=None)
def grid_case(kind, G):
    max_allele, missing = KINDS[kind]
    x, called = cohort(GRID_ROWS, GRID_COLS, max_allele, missing)
    masks = membership("halves", GRID_COLS, G, seed=7)
    blocks = [(0, GRID_ROWS), (1000, 5000)] + [(r, r + 1) for r in range(0, GRID_ROWS, 61)]
    return x, called, masks, blocks, fstat_ref.moments(x, called, masks, blocks)


@pytest.mark.parametrize("mask_bytes", ["1", None], ids=["masks=global", "masks=lds"])
@pytest.mark.parametrize("G", [5, 32])
@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_every_workgroup_takes_three_items(dev, fmh_opts, cus, kind, G, mask_bytes):
    """One row per item, more than three items for each of the at most 8 x CUs workgroups: the per-thread accumulators, the LDS counts and
    flags, the two tallies and the block's slice pointer are used a second and a third time."""
    max_allele, missing = KINDS[kind]
    x, called, masks, blocks, ref = grid_case(kind, G)
    assert GRID_ROWS > 3 * 8 * cus, f"{cus} CUs: {GRID_ROWS} one-row items no longer give every workgroup three"
    assert ref[0][0, 0] > 1000 and (ref[2][0] > 0) == missing and (ref[1][0] > 0) == (max_allele > 1)
    a, multi, incomplete = fstat_ref.classify(x, called, masks)
    flawed = multi | incomplete
    if missing:  # rows a grid apart alternate between flawed and usable: a flag or a count left behind would show
        assert (flawed[: GRID_ROWS - 8 * cus] & ~flawed[8 * cus:]).sum() > 50 and (~flawed[: GRID_ROWS - 8 * cus] & flawed[8 * cus:]).sum() > 50
    fmh_opts.setenv("FMH_FSTAT_ITEM_ROWS", "1")
    set_option(fmh_opts, "FMH_FSTAT_LDS_MASK_BYTES", mask_bytes)
    dm = upload(dev, x, called, max_allele, planes=missing)
    try:
        got = dev.fstat_moments(dm, masks, blocks)
        assert_moments_equal(got, ref, (kind, G, mask_bytes))
        one_row = dev.fstat_moments(dm, masks, [(r, r + 1) for r in range(3000, 3400)])
        assert np.array_equal(one_row.moments[:, 0] + one_row.multiallelic + one_row.incomplete, np.ones(400, dtype=np.uint64))
        assert_moments_equal(one_row, fstat_ref.moments(x, called, masks, [(r, r + 1) for r in range(3000, 3400)]), "one-row blocks")
    finally:
        dm.close()


# ---- a product above 2^32 --------------------------------------------------------------------------------------------------------------------
def test_a_product_above_two_to_the_32(dev):
    """65 537 columns, every allele 1, two groups of every column, 17 rows: a_0 a_1 = 65 537^2 = 2^32 + 2^17 + 1 in every row - a 32-bit
    multiply (or a 32-bit accumulator) loses the top."""
    rows, cols = 17, 65537
    x = np.ones((rows, cols), dtype=np.uint8)
    masks = np.ones((2, cols), dtype=bool)
    want = np.array([[rows, rows * cols, rows * cols, rows * cols * cols, rows * cols * cols, rows * cols * cols]], dtype=np.uint64)
    ref = fstat_ref.moments(x, None, masks, [(0, rows)])
    assert np.array_equal(ref[0], want) and cols * cols > 1 << 32
    dm = upload(dev, x, None, 1)
    try:
        got = dev.fstat_moments(dm, masks)  # default: one block, every row
        assert_moments_equal(got, ref, "65 537 x 65 537")
        three = np.concatenate([masks, masks[:1]])
        three[2, 1::2] = False  # 32 769 members
        assert_moments_equal(dev.fstat_moments(dm, three, [(3, 17), (0, 1)]), fstat_ref.moments(x, None, three, [(3, 17), (0, 1)]), "three groups")
    finally:
        dm.close()


# ---- refusals, in the header's order ---------------------------------------------------------------------------------------------------------
def test_refusals_in_order(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    cols, rows = 513, 17
    x, _ = cohort(rows, cols, 1, False)
    dm = upload(dev, x, None, 1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    two = np.ones((2, cols), dtype=np.uint8)
    three = np.ones((33, cols), dtype=np.uint8)
    nobody = two.copy()
    nobody[1] = 0
    good = np.array([(0, rows)], dtype=np.uint64)
    past = np.array([(0, rows), (3, rows + 1)], dtype=np.uint64)
    backwards = np.array([(9, 3)], dtype=np.uint64)
    table = dev.DeviceBuffer(dm.device, 8 * 561 * 2)

    def refused(status, text, m, masks, G, blocks, n_blocks, d_table):
        got = lib.fmh_fstat_moments(m, None if masks is None else ptr(masks), G, None if blocks is None else ptr(blocks), n_blocks, d_table, None, None)
        assert got == status and text.encode() in lib.fmh_last_error(), (got, lib.fmh_last_error())

    INVALID, UNSUPPORTED = _abi.FMH_ERR_INVALID, _abi.FMH_ERR_UNSUPPORTED
    try:
        # 1. NULL pointers - each ahead of everything after it (a wrong group count, an empty group, a bad block, no block)
        refused(INVALID, "NULL matrix", None, None, 1, None, 0, None)
        refused(INVALID, "h_column_mask is NULL", dm._h, None, 1, None, 0, None)
        refused(INVALID, "h_blocks is NULL", dm._h, nobody, 1, None, 0, None)
        refused(INVALID, "d_moments is NULL", dm._h, nobody, 1, backwards, 0, None)
        # 2. the group count, ahead of an empty group, a bad block and no block
        for G in (1, 0, -3, 33):
            refused(INVALID, "2 to 32 groups", dm._h, three if G == 33 else nobody, G, backwards, 0, table.ptr)
        # 3. a group with no member, ahead of a bad block and no block
        refused(INVALID, "group 1 has no member", dm._h, nobody, 2, backwards, 0, table.ptr)
        refused(INVALID, "group 1 has no member", dm._h, nobody, 2, past, 2, table.ptr)
        # 4. a block outside the matrix or backwards
        refused(INVALID, "exceed", dm._h, two, 2, past, 2, table.ptr)
        refused(INVALID, "exceed", dm._h, two, 2, backwards, 1, table.ptr)
        # 5. no block
        refused(INVALID, "n_blocks is 0", dm._h, two, 2, good, 0, table.ptr)
        # 6. a moment that could wrap: 2^45 rows x 513^2 >= 2^63, declared by a wrapped matrix over 1 KiB (nothing reads it: u8 rows only, so
        # the refusal after this one would be its lot as well)
        raw = dev.DeviceBuffer(dm.device, 1024)
        huge = dev.DeviceMatrix.wrap(raw.ptr, 528, None, 0, 1 << 45, cols, 1, 1)
        try:
            wide = np.array([(0, 1 << 45)], dtype=np.uint64)
            refused(UNSUPPORTED, "2^63", huge._h, two, 2, wide, 1, table.ptr)
            refused(INVALID, "exceed", huge._h, two, 2, np.array([(0, (1 << 45) + 1)], dtype=np.uint64), 1, table.ptr)  # 4 before 6
            narrow = np.array([(0, 1 << 44)], dtype=np.uint64)  # 2^44 x 513^2 < 2^63: on to refusal 7
            refused(UNSUPPORTED, "fmh_matrix_pack", huge._h, two, 2, narrow, 1, table.ptr)
            one_member = np.zeros((2, cols), dtype=np.uint8)
            one_member[:, 7] = 1
            refused(UNSUPPORTED, "fmh_matrix_pack", huge._h, one_member, 2, wide, 1, table.ptr)  # max(n) = 1: 2^45 rows are fine
        finally:
            huge.close()
        # the Python-side wrapper raises the same
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.fstat_moments(dm, nobody)
        assert err.value.status == INVALID and "no member" in str(err.value)
    finally:
        dm.close()
    # 7. a matrix without the packed image
    fmh_opts.setenv("FMH_LAYOUT", "bytes")
    dm = upload(dev, x, None, 1)
    try:
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.fstat_moments(dm, two)
        assert err.value.status == UNSUPPORTED and "fmh_matrix_pack" in str(err.value)
        dm.pack()
        assert_moments_equal(dev.fstat_moments(dm, two), fstat_ref.moments(x, None, two.astype(bool), [(0, rows)]), "after fmh_matrix_pack")
    finally:
        dm.close()


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------------
def haplotype_mask(haps):
    mask = np.zeros(12, dtype=bool)
    for s, side in haps:
        mask[2 * s + side] = True
    return mask


def assert_estimate(got, table, sizes, quad, unbiased=True):
    """An FStatEstimate against the oracle: the estimate within the block sums' bounds (tests/test_fstat_cpu.py), theta_J / se / z within 16
    times the deviation measured there, of the exact jackknife of the block sums the C code itself produced."""
    from ferromic_amd import device

    keep = [b for b in range(len(table)) if table[b][0] > 0]
    exact = [fstat_ref.f4(table[b], sizes, *quad, unbiased) for b in keep]
    sites = sum(int(table[b][0]) for b in keep)
    assert got.blocks == len(keep) and got.sites == sites
    if not keep:
        assert math.isnan(got.estimate)
        return
    bound = sum(e[1] + e[2] for e in exact) / (1 << 50) + len(keep) * sum(abs(e[0]) for e in exact) / (1 << 53)
    assert abs(Fraction(got.estimate) - sum(e[0] for e in exact) / sites) <= bound / sites + abs(Fraction(got.estimate)) / (1 << 52)
    sums = [device.fstat_f4(table[b], sizes, *quad, unbiased) for b in range(len(table))]
    ref = fstat_ref.jackknife(sums, [float(table[b][0]) for b in range(len(table))])
    if len(keep) < 2:
        assert math.isnan(got.se) and math.isnan(got.z)
        return
    for key, want in (("jackknife_estimate", ref["jackknife_estimate"]), ("se", Fraction(ref["se"])), ("z", Fraction(ref["z"]))):
        assert abs(Fraction(getattr(got, key)) - want) <= JACKKNIFE_MARGIN * JACKKNIFE_MEASURED[key] * abs(want), key


def test_python_f_statistics(fm):
    x, called, positions, records = python_cohort()  # 40 sites x 12 columns; site 5 carries an allele 2, site 9 an uncalled sample
    dense = np.where(called, x, -1).astype(np.int8).reshape(40, 6, 2)
    haps = [[(0, 0), (0, 1), (1, 0)], [(1, 1), (2, 0), (2, 1), (3, 0)], [(3, 1), (4, 0), (4, 1), (5, 0), (5, 1)], [(0, 0), (3, 0), (5, 1)]]
    masks = np.stack([haplotype_mask(h) for h in haps])
    sizes = masks.sum(axis=1).astype(np.uint64)
    everyone = sorted({h for group in haps for h in group})
    for make in (lambda h: fm.Population.from_numpy("d", dense, positions.astype(np.int64), h, 1000), lambda h: fm.Population("s", records, h, 1000)):
        base = make(everyone)
        pops = [base.with_haplotypes(g, h) for g, h in enumerate(haps)]
        # neither blocks nor block_size: one block over every row
        whole = fm.f_statistics(pops)
        ref = fstat_ref.moments(x, called, masks, [(0, 40)])
        assert ref[1][0] == 1 and ref[2][0] == 1 and ref[0][0, 0] == 38
        assert whole.sample_sizes == (3, 4, 5, 3) and whole.moments.shape == (1, 15) and np.array_equal(whole.moments, ref[0])
        assert np.array_equal(whole.multiallelic_sites, ref[1]) and np.array_equal(whole.incomplete_sites, ref[2]) and whole.usable_sites.tolist() == [38]
        assert_estimate(whole.f2(0, 1), ref[0], sizes, (0, 1, 0, 1))
        # blocks in the coordinates of the positions (100, 110, .., 490), inclusive at both ends; one is empty, two overlap
        blocks = [(100, 190), (400, 10**6), (0, 50), (180, 330), (95, 1000)]
        rows = [(0, 10), (30, 40), (0, 0), (8, 24), (0, 40)]
        got = fm.f_statistics(pops, blocks=blocks)
        ref = fstat_ref.moments(x, called, masks, rows)
        assert np.array_equal(got.moments, ref[0]) and np.array_equal(got.multiallelic_sites, ref[1]) and np.array_equal(got.incomplete_sites, ref[2])
        assert_estimate(got.f2(0, 1), ref[0], sizes, (0, 1, 0, 1))
        assert_estimate(got.f3(2, 0, 1), ref[0], sizes, (2, 0, 2, 1))
        assert_estimate(got.f4(0, 1, 2, 3), ref[0], sizes, (0, 1, 2, 3))
        assert_estimate(got.f4(0, 1, 2, 3, unbiased=False), ref[0], sizes, (0, 1, 2, 3), False)
        assert got.f2_blocks().shape == (5, 4, 4) and np.isnan(got.f2_blocks()[2]).all()
        # block_size in base pairs from the first position: [100, 169], [170, 239], .. = rows 0..6, 7..13, .., 35..39
        sized = fm.f_statistics(pops, block_size=70)
        rows = [(r, min(r + 7, 40)) for r in range(0, 40, 7)]
        ref = fstat_ref.moments(x, called, masks, rows)
        assert sized.moments.shape == (6, 15) and np.array_equal(sized.moments, ref[0]) and np.array_equal(sized.incomplete_sites, ref[2])
        assert_estimate(sized.f3(2, 0, 1), ref[0], sizes, (2, 0, 2, 1))
        assert_estimate(sized.f4(0, 1, 2, 3), ref[0], sizes, (0, 1, 2, 3))
        # concatenate of two calls == one call over both sets of blocks
        first, second = fm.f_statistics(pops, blocks=blocks[:2]), fm.f_statistics(pops, blocks=blocks[2:])
        joined = fm.FStatistics.concatenate([first, second])
        assert np.array_equal(joined.moments, got.moments) and np.array_equal(joined.multiallelic_sites, got.multiallelic_sites)
        assert np.array_equal(joined.incomplete_sites, got.incomplete_sites) and joined.sample_sizes == got.sample_sizes
        assert joined.f4(0, 1, 2, 3).z == got.f4(0, 1, 2, 3).z and joined.f2(1, 2).se == got.f2(1, 2).se
        with pytest.raises(ValueError) as err:
            fm.f_statistics([pops[0], make(haps[1])])  # equal variants, another resident matrix
        assert "ONE resident matrix" in str(err.value)
    # positions that do not ascend: a block's rows are then several runs, summed
    shuffled = records[20:] + records[:20]
    base = fm.Population("s", shuffled, everyone, 1000)
    got = fm.f_statistics([base.with_haplotypes(g, h) for g, h in enumerate(haps)], blocks=[(150, 350)])
    assert np.array_equal(got.moments, fstat_ref.moments(x, called, masks, [(5, 26)])[0])
