"""Linkage disequilibrium on the device (fmh_ld_band, fmh_ld_prune) against tests/ld_ref.py, the numpy oracle built on exact 0/1 matrix
products.  Counts must be equal, r^2 the same BITS (the definition leaves three roundings and no fused multiply-add), NaN positions and the
threshold words included - padding bits of the last word zero.

Shapes are the smallest at which each part of the kernel can go wrong: a partial last dword and last 16-byte vector, one and several K
slabs (256 bytes of a row per slab when nothing is missing, 128 otherwise), more than 65 535 columns, partial row tiles and d tiles,
partners beyond the rows asked for and beyond the matrix, bands around the 32-bit word and the 64-wide tile.  The ways a matrix can be
made (a foreign plane pitch, wrapped rows with junk padding, the generator, a re-pack in place) are covered by tests/test_gpu_cohort_fuzz.py.
"""

import functools

import numpy as np
import pytest

from tests import ld_ref
from tests.helpers import assert_bits_equal

pytestmark = pytest.mark.gpu


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
def cohort(rows, cols, max_allele, missing, seed):
    """(alleles [rows][cols] uint8, called [rows][cols] bool or None).  Neighbouring rows are copies with 20 % of the columns redrawn, so
    that r^2 spans 0..1; rows 3 and 5 are monomorphic; with missing calls row 7 is entirely uncalled and rows 10 / 11 share no called column."""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, cols), dtype=np.uint8)
    freq = rng.uniform(0.05, 0.95, size=rows)
    x[0] = rng.random(cols) < freq[0]
    for i in range(1, rows):
        x[i] = np.where(rng.random(cols) < 0.8, x[i - 1], rng.random(cols) < freq[i])
    if max_allele > 1:
        high = (x == 1) & (rng.random((rows, cols)) < 0.25)
        x[high] = rng.integers(2, max_allele + 1, size=int(high.sum()), dtype=np.uint8)
    if rows > 5:
        x[3] = 0
        x[5] = 1
    called = None
    if missing:
        called = rng.random((rows, cols)) >= 0.03
        if rows > 11:
            called[7] = False
            called[10, cols // 2:] = False
            called[11, : cols // 2] = False
    x.setflags(write=False)
    if called is not None:
        called.setflags(write=False)
    return x, called


def shape_of(cols):
    return (cols // 2, 2) if cols % 2 == 0 else (cols, 1)


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


def upload(dev, x, called, max_allele, planes=False, seed=0):
    """The cohort as a device matrix: through fmh_matrix_create, or (planes=True) as bit planes through fmh_matrix_create_packed with RANDOM
    bits under the uncalled entries of every allele plane - the kernel has to mask them with the called plane."""
    rows, cols = x.shape
    samples, ploidy = shape_of(cols)
    if not planes:
        data = x if called is None else np.where(called, x, 0).astype(np.uint8)
        return dev.DeviceMatrix.from_host(data, None if called is None else missing_words(called), rows, samples, ploidy, max_allele)
    rng = np.random.default_rng(seed + 99)
    pitch = ((cols + 7) // 8 + 15) // 16 * 16
    n_planes = 1 if max_allele <= 1 else 2 if max_allele <= 3 else 3
    stored = x.copy()
    if called is not None:
        junk = rng.integers(0, 1 << n_planes, size=x.shape, dtype=np.uint8)
        stored = np.where(called, x, junk).astype(np.uint8)
    bit_planes = [pack_rows((stored >> k) & 1, pitch) for k in range(n_planes)]
    return dev.DeviceMatrix.from_host_planes(bit_planes, None if called is None else pack_rows(called, pitch), rows, samples, ploidy, max_allele)


def column_mask(kind, cols, seed):
    if kind is None:
        return None
    rng = np.random.default_rng(seed + 5)
    if kind == "70%":
        return rng.random(cols) < 0.7
    mask = np.zeros(cols, dtype=bool)
    if kind == "vec3-5":  # members in the 16-byte vectors 3..5 of the row only (columns 384..767)
        mask[384:768] = rng.random(384) < 0.8
        mask[384] = mask[767] = True
    elif kind == "one":
        mask[cols // 3] = True
    return mask


def check_band(dev, x, called, max_allele, mask, row_begin, row_count, partner_end, band, threshold, planes=False, expect_spread=False):
    dm = upload(dev, x, called, max_allele, planes)
    g = None
    try:
        if mask is not None:
            g = dev.Groups(dm, mask[None, :].astype(np.uint8))
        got = dev.ld_band(dm, g, band, threshold, row_begin, row_count, partner_end)
        again = dev.ld_band(dm, g, band, threshold, row_begin, row_count, partner_end, want=("r2", "over"))
    finally:
        if g is not None:
            g.close()
        dm.close()
    ref = ld_ref.band(x, called, mask, row_begin, row_count, partner_end, band, threshold)
    for key in ("n_ab", "n_joint", "site_n", "site_alt"):
        assert np.array_equal(getattr(got, key), ref[key]), key
    assert_bits_equal(got.r2.reshape(-1), ref["r2"].reshape(-1), "r2")
    assert got.over.shape == ref["over"].shape and np.array_equal(got.over, ref["over"]), "over"
    assert np.array_equal(got.r2.view(np.uint64), again.r2.view(np.uint64)) and np.array_equal(got.over, again.over), "two calls, same bits"
    if expect_spread:  # the case is not vacuous: finite values on both sides of the threshold, and NaN entries
        finite = ref["r2"][np.isfinite(ref["r2"])]
        assert (finite > max(threshold, 0.5)).any() and (finite <= threshold).any() or threshold == 0.0
        assert np.isnan(ref["r2"]).any()


# ---- the band kernel ------------------------------------------------------------------------------------------------------------------
# columns, rows, band: every column count with both cores; row counts 1, 63, 65, 200; bands 1, 31, 32, 33, 64, 70 and one above the row count
BAND_SHAPES = [
    (1, 65, 31),
    (63, 200, 70),
    (64, 63, 64),
    (65, 65, 33),
    (130, 200, 32),
    (130, 1, 1),
    (130, 63, 100),
    (130, 200, 1),
    (5000, 200, 70),
    (70001, 65, 33),
]


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("cols,rows,band", BAND_SHAPES)
def test_band_biallelic(dev, cols, rows, band, missing):
    x, called = cohort(rows, cols, 1, missing, seed=cols + rows)
    check_band(dev, x, called, 1, None, 0, rows, rows, band, 0.3 if band != 32 else 0.0, expect_spread=rows >= 63 and cols >= 63 and band >= 31)


@pytest.mark.parametrize("max_allele", [3, 7])
@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("cols,rows,band", [(130, 200, 70), (5000, 65, 33)])
def test_band_multi_allelic_planes_with_bits_under_uncalled_entries(dev, cols, rows, band, missing, max_allele):
    x, called = cohort(rows, cols, max_allele, missing, seed=17 * max_allele + cols)
    assert x.max() == max_allele
    check_band(dev, x, called, max_allele, None, 0, rows, rows, band, 0.3, planes=True, expect_spread=True)


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("cols,kind", [(130, "70%"), (5000, "70%"), (5000, "vec3-5"), (5000, "one"), (130, "one")])
def test_band_membership_mask(dev, cols, kind, missing):
    x, called = cohort(200, cols, 1, missing, seed=cols + 3)
    mask = column_mask(kind, cols, seed=cols)
    if kind == "vec3-5":
        assert cols == 5000 and (cols + 127) // 128 == 40
    check_band(dev, x, called, 1, mask, 0, 200, 200, 70, 0.3, expect_spread=kind != "one")


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("row_begin,rows", [(0, 200), (37, 200), (37, 263)])
@pytest.mark.parametrize("to_matrix_end", [False, True], ids=["partners_end_with_rows", "partners_to_matrix_end"])
def test_band_row_range_and_partner_end(dev, row_begin, rows, to_matrix_end, missing):
    """Rows of a 300-row matrix: partners stop with the rows asked for, or reach beyond them (partner_end = variants); rows 37 .. 299 run
    their bands past the matrix end."""
    x, called = cohort(300, 130, 1, missing, seed=300)
    check_band(dev, x, called, 1, None, row_begin, rows, 300 if to_matrix_end else row_begin + rows, 70, 0.3, expect_spread=True)


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
def test_band_many_tiles(dev, missing):
    """2 000 rows x 130 columns, band 200: 32 row tiles x 4 d tiles, the last of each partial."""
    x, called = cohort(2000, 130, 1, missing, seed=2000)
    check_band(dev, x, called, 1, column_mask("70%", 130, 1) if missing else None, 0, 2000, 2000, 200, 0.2, expect_spread=True)


def test_band_only_some_outputs_and_no_rows(dev):
    x, called = cohort(65, 130, 1, True, seed=65)
    dm = upload(dev, x, called, 1)
    try:
        got = dev.ld_band(dm, None, 33, 0.3, want=("n_joint",))
        assert got.r2 is None and got.over is None and got.site_n is None
        assert np.array_equal(got.n_joint, ld_ref.band(x, called, None, 0, 65, 65, 33, 0.3)["n_joint"])
        empty = dev.ld_band(dm, None, 33, 0.3, row_begin=10, row_count=0)
        assert empty.r2.shape == (0, 33)
    finally:
        dm.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, fmh_opts):
    from ferromic_amd import _abi

    x, _ = cohort(65, 130, 1, False, seed=65)
    dm = upload(dev, x, None, 1)
    two = dev.Groups(dm, np.stack([np.ones(130, np.uint8), np.zeros(130, np.uint8)]))
    try:
        for kwargs, g in ((dict(band=0), None), (dict(band=3, partner_end=66), None), (dict(band=3, row_begin=60, row_count=10), None), (dict(band=3), two),
                          (dict(band=3, threshold=float("nan")), None)):
            with pytest.raises(_abi.FerromicHipError) as err:
                dev.ld_band(dm, g, **kwargs)
            assert err.value.status == _abi.FMH_ERR_INVALID, kwargs
        assert _abi.load().fmh_ld_band(dm._h, None, 0, 65, 65, 3, 0.5, None, None, None, None) == _abi.FMH_ERR_INVALID  # NULL output struct
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.ld_prune(dm, two, 3, 0.5)
        assert err.value.status == _abi.FMH_ERR_INVALID
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.ld_prune(dm, None, 0, 0.5)
        assert err.value.status == _abi.FMH_ERR_INVALID
    finally:
        two.close()
        dm.close()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    dm = upload(dev, x, None, 1)
    try:
        for call in (lambda: dev.ld_band(dm, None, 3), lambda: dev.ld_prune(dm, None, 3, 0.5)):
            with pytest.raises(_abi.FerromicHipError) as err:
                call()
            assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and "fmh_matrix_pack" in str(err.value)
        dm.pack()
        assert dev.ld_band(dm, None, 3, want=("r2",)).r2.shape == (65, 3)
    finally:
        dm.close()


# ---- pruning ----------------------------------------------------------------------------------------------------------------------------
PRUNE_WINDOW = 50


@functools.lru_cache(maxsize=None)
def prune_case(rows):
    x, called = cohort(rows, 130, 1, rows == 200, seed=rows + 1)
    return x, called, ld_ref.band(x, called, None, 0, rows, rows, PRUNE_WINDOW, 0.0)["r2"]


@pytest.mark.parametrize("threshold", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("rows,chunk", [(200, 0), (200, 77), (5000, 0), (5000, 777)])
def test_prune_equals_the_bits_rule_and_the_oracle(dev, rows, chunk, threshold):
    """fmh_ld_prune (chunk 0: the library's chunk length; 77 / 777 rows: several chunks, pairs reaching across their boundaries) = the greedy
    rule over the `over` band of ONE fmh_ld_band call = the oracle's greedy over its own r^2."""
    x, called, r2 = prune_case(rows)
    dm = upload(dev, x, called, 1)
    try:
        keep = dev.ld_prune(dm, None, PRUNE_WINDOW, threshold, chunk_rows=chunk)
        over = dev.ld_band(dm, None, PRUNE_WINDOW, threshold, want=("over",)).over
    finally:
        dm.close()
    expected = ld_ref.greedy_from_r2(r2, threshold)
    assert np.array_equal(dev.ld_prune_bits(over, PRUNE_WINDOW), expected)
    assert np.array_equal(keep, expected)
    if threshold == 1.0:
        assert keep.all()
    elif threshold == 0.2:
        assert 0 < keep.sum() < rows


def test_prune_row_range_with_a_group(dev):
    x, called = cohort(300, 130, 1, True, seed=300)
    mask = column_mask("70%", 130, 2)
    dm = upload(dev, x, called, 1)
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    try:
        keep = dev.ld_prune(dm, g, 40, 0.2, row_begin=37, row_count=200, chunk_rows=64)
    finally:
        g.close()
        dm.close()
    r2 = ld_ref.band(x, called, mask, 37, 200, 237, 40, 0.2)["r2"]
    assert np.array_equal(keep, ld_ref.greedy_from_r2(r2, 0.2))


# ---- through `import ferromic` --------------------------------------------------------------------------------------------------------
def test_population_from_numpy(fm):
    """300 sites x 40 diploid samples with missing calls, a haplotype subset: Population.ld_r2 / ld_prune on the resident matrix."""
    rng = np.random.default_rng(40)
    x, called = cohort(300, 80, 1, True, seed=40)
    geno = np.where(called, x, -1).astype(np.int8).reshape(300, 40, 2)
    haps = [(int(s), int(side)) for s in rng.choice(40, size=25, replace=False) for side in (0, 1)][:-3]
    mask = np.zeros(80, dtype=bool)
    for s, side in haps:
        mask[2 * s + side] = True
    pop = fm.Population.from_numpy("p", geno, np.arange(300, dtype=np.int64) * 7, haps, 3000)
    r2 = pop.ld_r2(33)
    ref = ld_ref.band(x, called, mask, 0, 300, 300, 33, 0.0)["r2"]
    assert isinstance(r2, np.ndarray) and r2.dtype == np.float64 and r2.shape == (300, 33)
    assert_bits_equal(r2.reshape(-1), ref.reshape(-1), "Population.ld_r2")
    keep = pop.ld_prune(33, 0.2)
    assert keep.dtype == bool and np.array_equal(keep, ld_ref.greedy_from_r2(ref, 0.2))
    assert 0 < keep.sum() < 300


def test_ld_r2_of_a_variant_list_with_a_region(fm):
    """A sparse variant list (records with missing genotypes) and a region that cuts rows off both ends."""
    x, called = cohort(60, 24, 1, True, seed=24)
    variants = []
    for i in range(60):
        calls = []
        for s in range(12):
            if not called[i, 2 * s]:
                calls.append(None)  # a missing genotype: neither allele is called
            else:
                calls.append([int(x[i, 2 * s]), int(x[i, 2 * s + 1])])
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    haps = [(s, side) for s in range(1, 11) for side in (0, 1)]
    mask = np.zeros(24, dtype=bool)
    mask[2:22] = True
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    r2 = fm.ld_r2(variants, haps, 9, region=region)
    ref = ld_ref.band(x[6:52], eff_called[6:52], mask, 0, 46, 46, 9, 0.0)["r2"]
    assert r2.shape == (46, 9)
    assert_bits_equal(r2.reshape(-1), ref.reshape(-1), "ld_r2 with a region")
    keep = fm.ld_prune(variants, haps, 9, 0.3, region=region)
    assert np.array_equal(keep, ld_ref.greedy_from_r2(ref, 0.3))
    whole = fm.ld_r2(variants, haps, 9)
    assert whole.shape == (60, 9)
    assert_bits_equal(whole.reshape(-1), ld_ref.band(x, eff_called, mask, 0, 60, 60, 9, 0.0)["r2"].reshape(-1), "ld_r2 without a region")
