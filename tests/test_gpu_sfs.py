"""Site frequency spectra on the device (fmh_sfs, fmh_sfs_joint) against tests/sfs_ref.py, the numpy oracle written from the definition.
Every comparison is array_equal on integers: tables, tallies, and the same table again under every route (LDS tile size, rows per item,
row tables on or off, windows asked for together or one call at a time).

Shapes are the smallest at which each part of the kernel can go wrong: a partial last dword and last 16-byte vector, rows of one to five
vectors (four lanes per row up to four vectors, sixteen beyond), row counts around the 16 and 64 rows a pass of a workgroup takes, 300 rows
for several items and passes, tiles smaller than the table (the corner mapping and the global path), and one spectrum one bin wider than
the tile, at the default cap and at the largest (the 512-thread launch).

Cohorts: allele frequencies skewed to rare alleles, monomorphic rows of both kinds, and - so that wide groups still have usable rows - the
missing calls (3 % of all entries) and the alleles above 1 sit in a third of the rows each; with missing calls one row is entirely uncalled.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import sfs_ref

pytestmark = pytest.mark.gpu

COLUMNS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 513]
ROWS = [1, 3, 4, 5, 15, 16, 17, 300]
# (max_allele, missing)
KINDS = {"complete": (1, False), "missing": (1, True), "multi3-missing": (3, True), "multi7": (7, False)}


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


# ---- cohorts ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cohort(rows, cols, max_allele, missing, seed=0):
    """(alleles [rows][cols] uint8, called [rows][cols] bool or None), read-only and shared between the tests."""
    rng = np.random.default_rng(1000003 * rows + 7919 * cols + 31 * max_allele + missing + seed)
    freq = rng.beta(0.35, 1.6, size=rows)  # most rows rare, a tail of common ones
    x = (rng.random((rows, cols)) < freq[:, None]).astype(np.uint8)
    if rows > 5:
        x[2] = 0
        x[4] = 1
    if max_allele > 1:
        some = rng.random(rows) < 1 / 3
        if rows > 1:
            some[1] = True
        high = (x == 1) & some[:, None] & (rng.random((rows, cols)) < 0.25)
        x[high] = rng.integers(2, max_allele + 1, size=int(high.sum()), dtype=np.uint8)
        if rows > 1 and cols > 2:
            x[1, cols // 2] = max_allele
    called = None
    if missing:
        some = rng.random(rows) < 1 / 3
        called = ~(some[:, None] & (rng.random((rows, cols)) < 0.09))
        if rows > 3:
            called[3] = False  # one all-uncalled row
    x.setflags(write=False)
    if called is not None:
        called.setflags(write=False)
    return x, called


def missing_words(called):
    flat = ~called.reshape(-1)
    padded = np.zeros((flat.size + 63) // 64 * 64, dtype=np.uint8)
    padded[: flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def pack_rows(bits, pitch):
    rows, cols = bits.shape
    padded = np.zeros((rows, pitch * 8), dtype=np.uint8)
    padded[:, :cols] = bits
    return np.packbits(padded, axis=1, bitorder="little")


def upload(dev, x, called, max_allele, planes=False, ploidy=None):
    """Through fmh_matrix_create, or (planes=True) as bit planes through fmh_matrix_create_packed with RANDOM bits under the uncalled entries
    of every allele plane - the kernel has to mask them with the called plane."""
    rows, cols = x.shape
    if ploidy is None:
        ploidy = 2 if cols % 2 == 0 else 1
    samples = cols // ploidy
    if not planes:
        data = x if called is None else np.where(called, x, 0).astype(np.uint8)
        return dev.DeviceMatrix.from_host(data, None if called is None else missing_words(called), rows, samples, ploidy, max_allele)
    rng = np.random.default_rng(rows + cols + 99)
    pitch = ((cols + 7) // 8 + 15) // 16 * 16
    n_planes = 1 if max_allele <= 1 else 2 if max_allele <= 3 else 3
    stored = x.copy()
    if called is not None:
        junk = rng.integers(0, 1 << n_planes, size=x.shape, dtype=np.uint8)
        stored = np.where(called, x, junk).astype(np.uint8)
    bit_planes = [pack_rows((stored >> k) & 1, pitch) for k in range(n_planes)]
    return dev.DeviceMatrix.from_host_planes(bit_planes, None if called is None else pack_rows(called, pitch), rows, samples, ploidy, max_allele)


def group_masks(cols, seed):
    """all columns; a single member; members only in the last (partial) 16-byte vector; a random half"""
    rng = np.random.default_rng(cols + seed)
    one = np.zeros(cols, dtype=bool)
    one[cols // 3] = True
    last = np.zeros(cols, dtype=bool)
    first_of_last = (cols - 1) // 128 * 128
    last[first_of_last:] = rng.random(cols - first_of_last) < 0.6
    last[cols - 1] = True
    half = rng.random(cols) < 0.5
    half[rng.integers(cols)] = True
    return {"all": np.ones(cols, dtype=bool), "one": one, "last-vector": last, "half": half}


def run_sfs(dev, dm, mask, windows):
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    try:
        return dev.sfs(dm, g, windows)
    finally:
        g.close()


def run_joint(dev, dm, mask0, mask1, row_begin=0, row_count=None):
    g = dev.Groups(dm, np.stack([mask0, mask1]).astype(np.uint8))
    try:
        return dev.sfs_joint(dm, g, row_begin, row_count)
    finally:
        g.close()


def assert_sfs_equal(got, ref, what):
    counts, multi, incomplete = ref
    assert got.counts.dtype == np.uint64 and got.counts.shape == counts.shape, what
    assert np.array_equal(got.counts, counts), what
    assert np.array_equal(got.multiallelic, multi) and np.array_equal(got.incomplete, incomplete), what


# ---- geometry x matrix kinds x row tables -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2", None], ids=["row_hi=0", "row_hi=2", "row_hi=default"])
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_geometry_and_group(dev, fmh_opts, kind, planes, row_hi):
    max_allele, missing = KINDS[kind]
    if row_hi is not None:
        fmh_opts.setenv("FMH_ROW_HI", row_hi)
    seen_multi = seen_incomplete = 0
    interior = set()
    for cols in COLUMNS:
        masks = group_masks(cols, 3)
        for rows in ROWS:
            for ploidy in ((1, 2) if cols % 2 == 0 and rows in (5, 300) else (None,)):
                x, called = cohort(rows, cols, max_allele, missing)
                dm = upload(dev, x, called, max_allele, planes, ploidy)
                try:
                    windows = [(0, rows), (rows // 2, rows)]
                    for name, mask in masks.items():
                        ref = sfs_ref.sfs(x, called, mask, windows)
                        got = run_sfs(dev, dm, mask, windows)
                        assert_sfs_equal(got, ref, (cols, rows, ploidy, name))
                        # every row is accounted for
                        assert int(got.counts[0].sum() + got.multiallelic[0] + got.incomplete[0]) == rows
                        seen_multi += int(ref[1][0])
                        seen_incomplete += int(ref[2][0])
                        n = int(mask.sum())
                        interior.update((n, int(k)) for k in np.nonzero(ref[0][0][1:n])[0])
                    # the joint spectrum of two overlapping groups of different sizes, and of a group with itself
                    if cols >= 2:
                        for a, b in (("half", "last-vector"), ("all", "one"), ("half", "half")):
                            ref = sfs_ref.sfs_joint(x, called, masks[a], masks[b], 0, rows)
                            got = run_joint(dev, dm, masks[a], masks[b])
                            assert np.array_equal(got.counts, ref[0]) and (got.multiallelic, got.incomplete) == ref[1:], (cols, rows, a, b)
                            assert int(got.counts.sum()) + got.multiallelic + got.incomplete == rows
                finally:
                    dm.close()
    # not vacuous (from the oracle): interior bins hit, and the tallies the kind is about
    assert len(interior) >= 3
    assert (seen_incomplete > 0) == missing and (seen_multi > 0) == (max_allele > 1)


# ---- routes: tile smaller than the table, rows per item -----------------------------------------------------------------------------
def members(cols, n, seed):
    mask = np.zeros(cols, dtype=bool)
    mask[np.random.default_rng(seed).choice(cols, size=n, replace=False)] = True
    return mask


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
@pytest.mark.parametrize("n", [40, 257])
def test_lds_tile_smaller_than_the_table(dev, fmh_opts, kind, n):
    max_allele, missing = KINDS[kind]
    cols, rows = 513, 300
    x, called = cohort(rows, cols, max_allele, missing, seed=n)
    mask = members(cols, n, n)
    windows = [(0, rows), (10, 200), (299, 300)]
    ref = sfs_ref.sfs(x, called, mask, windows)
    assert len(np.nonzero(ref[0][0][1:n])[0]) >= 3
    if missing:
        assert ref[1][0] > 0 and ref[2][0] > 0
    dm = upload(dev, x, called, max_allele, planes=missing)
    try:
        tables = []
        for bins in ("4", "8", "64", None):
            if bins is not None:
                fmh_opts.setenv("FMH_SFS_LDS_BINS", bins)
                if int(bins) < n + 1:  # the tile is smaller than the table: keys with min(k, n - k) < T stay on chip
                    T = int(bins) // 2
                    k = np.arange(n + 1)
                    inside = np.minimum(k, n - k) < T
                    assert ref[0][0][inside].any() and ref[0][0][~inside].any(), "the case exercises both the tile and the global path"
            else:
                fmh_opts.delenv("FMH_SFS_LDS_BINS")
            got = run_sfs(dev, dm, mask, windows)
            assert_sfs_equal(got, ref, bins)
            tables.append(got.counts)
        assert all(np.array_equal(tables[0], t) for t in tables[1:])
    finally:
        dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_joint_corners(dev, fmh_opts, kind):
    """33 x 20 members, overlapping; tiles of 16 and 64 bins hold the corners (2 x 2 and 4 x 4 keys at each), the rest goes to the table directly"""
    max_allele, missing = KINDS[kind]
    cols, rows = 129, 300
    x, called = cohort(rows, cols, max_allele, missing, seed=5)
    m0, m1 = members(cols, 33, 1), members(cols, 20, 2)
    assert (m0 & m1).any() and (m0 & ~m1).any()
    ref = sfs_ref.sfs_joint(x, called, m0, m1, 0, rows)
    if missing:
        assert ref[1] > 0 and ref[2] > 0
    dm = upload(dev, x, called, max_allele, planes=missing)
    try:
        tables = []
        for bins in ("16", "64", None):
            if bins is not None:
                fmh_opts.setenv("FMH_SFS_LDS_BINS", bins)
                T = int(np.sqrt(int(bins))) // 2  # a square tile: both axes are longer than its side
                k0, k1 = np.arange(34)[:, None], np.arange(21)[None, :]
                inside = (np.minimum(k0, 33 - k0) < T) & (np.minimum(k1, 20 - k1) < T)
                assert ref[0][inside].any() and ref[0][~inside].any()
            else:
                fmh_opts.delenv("FMH_SFS_LDS_BINS")
            got = run_joint(dev, dm, m0, m1)
            assert np.array_equal(got.counts, ref[0]) and (got.multiallelic, got.incomplete) == ref[1:], bins
            tables.append(got.counts)
        assert all(np.array_equal(tables[0], t) for t in tables[1:])
        part = run_joint(dev, dm, m0, m1, 7, 250)
        ref_part = sfs_ref.sfs_joint(x, called, m0, m1, 7, 250)
        assert np.array_equal(part.counts, ref_part[0]) and (part.multiallelic, part.incomplete) == ref_part[1:]
        empty = run_joint(dev, dm, m0, m1, 300, 0)
        assert not empty.counts.any() and empty.counts.shape == (34, 21)
    finally:
        dm.close()


@pytest.mark.parametrize("cap", ["default", "largest"])
def test_one_column_more_than_the_tile_holds(dev, fmh_opts, cap):
    """n + 1 bins = the tile cap + 1, at the default cap and at the largest the option takes (one 512-thread workgroup per CU, 160 KiB of
    LDS): the ends of the axis stay on chip and exactly one key - the middle one - goes to the table directly.  Rows are crafted at and
    around that key."""
    n = dev.SFS_DEFAULT_LDS_BINS if cap == "default" else dev.SFS_MAX_LDS_BINS
    if cap == "largest":
        fmh_opts.setenv("FMH_SFS_LDS_BINS", str(n))
    rows, T = 40, n // 2
    rng = np.random.default_rng(8)
    x = (rng.random((rows, n)) < rng.beta(0.35, 1.6, size=rows)[:, None]).astype(np.uint8)
    for r, k in ((0, T), (1, T - 1), (2, T + 1), (3, T), (4, 0), (5, n), (6, 1), (7, n - 1)):
        x[r] = 0
        x[r, rng.choice(n, size=k, replace=False)] = 1
    mask = np.ones(n, dtype=bool)
    ref = sfs_ref.sfs(x, None, mask, [(0, rows)])
    k = np.arange(n + 1)
    inside = np.minimum(k, n - k) < T
    assert (~inside).sum() == 1 and ref[0][0][~inside].sum() == 2 and ref[0][0][inside].any()
    dm = upload(dev, x, None, 1)
    try:
        assert_sfs_equal(run_sfs(dev, dm, mask, [(0, rows)]), ref, cap)
        if cap == "largest":  # one bin fewer than the cap: the whole axis on chip, still the 512-thread launch
            ref = sfs_ref.sfs(x, None, mask[:-1].tolist() + [False], [(0, rows)])
            assert_sfs_equal(run_sfs(dev, dm, np.array(mask[:-1].tolist() + [False]), [(0, rows)]), ref, "whole axis")
    finally:
        dm.close()


# ---- windows and items on 300 rows ------------------------------------------------------------------------------------------------------
WINDOW_SETS = {
    "whole": [(0, 300)],
    "one-row": [(r, r + 1) for r in range(0, 300, 7)],
    "empty": [(0, 0), (150, 150), (300, 300), (0, 300)],
    "overlapping-unordered": [(200, 300), (0, 120), (100, 250), (100, 250), (17, 18)],
    "to-the-last-row": [(299, 300), (236, 300)],
}


@pytest.mark.parametrize("item_rows", ["1", "5", "16", None], ids=["item=1", "item=5", "item=16", "item=default"])
@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_windows_and_items(dev, fmh_opts, kind, item_rows):
    max_allele, missing = KINDS[kind]
    cols, rows = 257, 300
    x, called = cohort(rows, cols, max_allele, missing, seed=11)
    mask = group_masks(cols, 11)["half"]
    if item_rows is not None:
        fmh_opts.setenv("FMH_SFS_ITEM_ROWS", item_rows)
    dm = upload(dev, x, called, max_allele, planes=True)
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    try:
        for name, windows in WINDOW_SETS.items():
            ref = sfs_ref.sfs(x, called, mask, windows)
            got = dev.sfs(dm, g, windows)
            assert_sfs_equal(got, ref, name)
            widths = np.array([e - b for b, e in windows], dtype=np.uint64)
            assert np.array_equal(got.counts.sum(axis=1) + got.multiallelic + got.incomplete, widths), name
            for w, window in enumerate(windows):  # the same windows, one call at a time
                one = dev.sfs(dm, g, [window])
                assert np.array_equal(one.counts[0], got.counts[w]) and one.multiallelic[0] == got.multiallelic[w] and one.incomplete[0] == got.incomplete[w]
        whole = dev.sfs(dm, g)  # default: one window, every row
        assert_sfs_equal(whole, sfs_ref.sfs(x, called, mask, [(0, rows)]), "default window")
    finally:
        g.close()
        dm.close()


# ---- invariants -----------------------------------------------------------------------------------------------------------------------------
def test_marginals_and_population_summaries_on_a_complete_matrix(dev):
    cols, rows = 257, 300
    x, _ = cohort(rows, cols, 1, False, seed=21)
    m0, m1 = members(cols, 40, 3), members(cols, 101, 4)
    dm = upload(dev, x, None, 1)
    g = dev.Groups(dm, np.stack([m0, m1]).astype(np.uint8))
    try:
        joint = dev.sfs_joint(dm, g)
        assert joint.multiallelic == 0 and joint.incomplete == 0
        for axis, mask in ((0, m0), (1, m1)):
            one = run_sfs(dev, dm, mask, [(0, rows)])
            assert np.array_equal(joint.counts.sum(axis=1 - axis), one.counts[0])
            stats = dev.sfs_stats(one.counts[0])
            totals = dev.population_summaries(dm, g, want_sites=False).totals[axis]
            assert stats["sites"] == rows and stats["segregating_sites"] == totals["segregating_sites"] > 3
            assert abs(stats["pi_sum"] - totals["pi_sum"]) <= 1e-9 * abs(totals["pi_sum"])
    finally:
        g.close()
        dm.close()


# ---- refusals on a live matrix ------------------------------------------------------------------------------------------------------------
def test_refusals(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, _ = cohort(17, 513, 1, False)
    everyone = np.ones((1, 513), dtype=np.uint8)
    dm = upload(dev, x, None, 1)
    other = upload(dev, cohort(17, 65, 1, False)[0], None, 1)
    g = dev.Groups(dm, everyone)
    two = dev.Groups(dm, np.concatenate([everyone, everyone]))
    nobody = dev.Groups(dm, np.zeros((1, 513), dtype=np.uint8))
    half_nobody = dev.Groups(dm, np.concatenate([everyone, np.zeros((1, 513), dtype=np.uint8)]))
    foreign = dev.Groups(other, np.ones((1, 65), dtype=np.uint8))
    try:
        def refused(call, status, text):
            with pytest.raises(_abi.FerromicHipError) as err:
                call()
            assert err.value.status == status and text in str(err.value), str(err.value)

        refused(lambda: dev.sfs(dm, two), _abi.FMH_ERR_INVALID, "exactly 1 group")
        refused(lambda: dev.sfs_joint(dm, g), _abi.FMH_ERR_INVALID, "exactly 2 groups")
        refused(lambda: dev.sfs(dm, foreign), _abi.FMH_ERR_INVALID, "not made for this matrix")
        refused(lambda: dev.sfs(dm, nobody), _abi.FMH_ERR_INVALID, "no member")
        refused(lambda: dev.sfs_joint(dm, half_nobody), _abi.FMH_ERR_INVALID, "no member")
        refused(lambda: dev.sfs(dm, g, [(0, 17), (3, 18)]), _abi.FMH_ERR_INVALID, "exceed")  # past the end
        refused(lambda: dev.sfs(dm, g, [(9, 3)]), _abi.FMH_ERR_INVALID, "exceed")          # begin > end
        refused(lambda: dev.sfs_joint(dm, two, 10, 8), _abi.FMH_ERR_INVALID, "exceed")
        refused(lambda: dev.sfs(dm, g, np.zeros((0, 2), dtype=np.uint64)), _abi.FMH_ERR_INVALID, "n_windows")
        # an oversize table, asked for with many (empty) windows: refused before anything of that size exists
        n_windows = (1 << 28) // 514 + 1
        windows = np.zeros((n_windows, 2), dtype=np.uint64)
        small = dev.DeviceBuffer(dm.device, 514 * 8)
        status = lib.fmh_sfs(dm._h, g._h, windows.ctypes.data_as(C.c_void_p), n_windows, small.ptr, None, None)
        assert status == _abi.FMH_ERR_UNSUPPORTED and b"2^28" in lib.fmh_last_error()
        assert lib.fmh_sfs(dm._h, g._h, windows.ctypes.data_as(C.c_void_p), n_windows - 1, None, None, None) == _abi.FMH_ERR_INVALID
    finally:
        for h in (g, two, nobody, half_nobody, foreign, dm, other):
            h.close()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    dm = upload(dev, x, None, 1)
    g = dev.Groups(dm, everyone)
    two = dev.Groups(dm, np.concatenate([everyone, everyone]))
    try:
        for call in (lambda: dev.sfs(dm, g), lambda: dev.sfs_joint(dm, two)):
            with pytest.raises(_abi.FerromicHipError) as err:
                call()
            assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and "fmh_matrix_pack" in str(err.value)
        dm.pack()
        assert_sfs_equal(dev.sfs(dm, g), sfs_ref.sfs(x, None, np.ones(513, dtype=bool), [(0, 17)]), "after fmh_matrix_pack")
    finally:
        g.close()
        two.close()
        dm.close()


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------------
def python_cohort():
    """40 sites x 6 diploid samples as variant records: site 5 carries an allele 2, site 9 has a sample without a genotype."""
    rng = np.random.default_rng(77)
    sites, samples = 40, 6
    x = (rng.random((sites, samples * 2)) < rng.beta(0.5, 1.2, size=sites)[:, None]).astype(np.uint8)
    x[5, 3] = 2
    called = np.ones(x.shape, dtype=bool)
    called[9, 4:6] = False
    positions = 100 + 10 * np.arange(sites)
    records = []
    for i in range(sites):
        genotypes = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(samples)]
        records.append(dict(position=int(positions[i]), genotypes=genotypes))
    return x, called, positions, records


def test_python_site_frequency_spectrum_of_variant_records(fm):
    x, called, positions, records = python_cohort()
    haps = [(0, 0), (0, 1), (2, 0), (2, 1), (3, 1), (5, 0)]
    mask = np.zeros(12, dtype=bool)
    for s, side in haps:
        mask[2 * s + side] = True
    whole = fm.site_frequency_spectrum(records, haps)
    ref = sfs_ref.sfs(x, called, mask, [(0, 40)])
    assert whole.sample_size == 6 and whole.counts.shape == (7,) and np.array_equal(whole.counts, ref[0][0])
    assert (whole.multiallelic_sites, whole.incomplete_sites) == (int(ref[1][0]), int(ref[2][0]))
    assert whole.segregating_sites == sfs_ref.stats(ref[0][0])["segregating_sites"] and isinstance(whole.tajimas_d, float)
    every = [(s, side) for s in range(6) for side in (0, 1)]
    ref_all = sfs_ref.sfs(x, called, np.ones(12, dtype=bool), [(0, 40)])
    got_all = fm.site_frequency_spectrum(records, every)
    assert np.array_equal(got_all.counts, ref_all[0][0]) and got_all.multiallelic_sites == 1 and got_all.incomplete_sites == 1
    # region = positions 150..300 inclusive = rows 5..20; windows in the same coordinates, clipped by the region
    region = fm.site_frequency_spectrum(records, every, region=(150, 300))
    assert np.array_equal(region.counts, sfs_ref.sfs(x, called, np.ones(12, dtype=bool), [(5, 21)])[0][0]) and region.multiallelic_sites == 1
    windows = [(100, 190), (400, 10**6), (0, 50), (180, 230), (95, 1000)]
    rows = [(0, 10), (30, 40), (0, 0), (8, 14), (0, 40)]
    got = fm.site_frequency_spectrum(records, haps, windows=windows)
    ref = sfs_ref.sfs(x, called, mask, rows)
    assert got.counts.shape == (5, 7) and np.array_equal(got.counts, ref[0])
    assert np.array_equal(got.multiallelic_sites, ref[1]) and np.array_equal(got.incomplete_sites, ref[2])
    assert got.segregating_sites.tolist() == [sfs_ref.stats(r)["segregating_sites"] for r in ref[0]]
    both = fm.site_frequency_spectrum(records, haps, region=(150, 300), windows=[(100, 190), (290, 500)])
    assert np.array_equal(both.counts, sfs_ref.sfs(x, called, mask, [(5, 10), (19, 21)])[0])
    # positions that do not ascend: a window's rows are then several runs, summed
    shuffled = records[20:] + records[:20]
    got = fm.site_frequency_spectrum(shuffled, haps, windows=[(150, 350)])
    assert np.array_equal(got.counts[0], sfs_ref.sfs(x, called, mask, [(5, 26)])[0][0])


def test_python_population_spectra(fm):
    x, called, positions, records = python_cohort()
    dense = np.where(called, x, -1).astype(np.int8).reshape(40, 6, 2)
    h1 = [(s, side) for s in (0, 1, 2) for side in (0, 1)]
    h2 = [(s, side) for s in (2, 3, 4, 5) for side in (0, 1)][1:]  # overlaps h1 in one haplotype, 7 members
    m1, m2 = np.zeros(12, dtype=bool), np.zeros(12, dtype=bool)
    for s, side in h1:
        m1[2 * s + side] = True
    for s, side in h2:
        m2[2 * s + side] = True
    for make in (lambda h: fm.Population.from_numpy("d", dense, positions.astype(np.int64), h, 1000), lambda h: fm.Population("s", records, h, 1000)):
        base = make(h1 + h2)
        p1, p2 = base.with_haplotypes(0, h1), base.with_haplotypes(1, h2)
        got = p1.site_frequency_spectrum()
        ref = sfs_ref.sfs(x, called, m1, [(0, 40)])
        assert got.sample_size == 6 and np.array_equal(got.counts, ref[0][0])
        assert (got.multiallelic_sites, got.incomplete_sites) == (int(ref[1][0]), int(ref[2][0]))
        got = p2.site_frequency_spectrum(windows=[(100, 290), (300, 1000)])
        ref = sfs_ref.sfs(x, called, m2, [(0, 20), (20, 40)])
        assert np.array_equal(got.counts, ref[0]) and np.array_equal(got.multiallelic_sites, ref[1]) and np.array_equal(got.incomplete_sites, ref[2])
        joint = fm.joint_site_frequency_spectrum(p1, p2)
        ref = sfs_ref.sfs_joint(x, called, m1, m2, 0, 40)
        assert joint.sample_sizes == (6, 7) and joint.counts.shape == (7, 8) and np.array_equal(joint.counts, ref[0])
        assert (joint.multiallelic_sites, joint.incomplete_sites) == ref[1:] and ref[1] == 1 and ref[2] == 1
        assert np.array_equal(joint.marginal(0), ref[0].sum(axis=1)) and np.array_equal(joint.marginal(1), ref[0].sum(axis=0))
        with pytest.raises(ValueError) as err:
            fm.joint_site_frequency_spectrum(p1, make(h2))  # equal variants, another resident matrix
        assert "ONE resident matrix" in str(err.value)
