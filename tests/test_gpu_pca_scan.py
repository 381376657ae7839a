"""The PCA site scan (fmh_pca_scan_sites) and the gather of fmh_pca_gram on what a real chromosome looks like: matrices with a called
plane, upper planes and the per-row tables row_gap / row_hi, rows of more than 4 096 columns, row ranges, kept rows between dirty ones.

Scan: per row the called allele-1 count and two flags against numpy, all integers, all equal.  The packed kernel skips the called plane
of rows row_gap marks complete and the upper planes of rows row_hi marks biallelic; the tables exist by default only from 4 096 rows up,
so every cohort is uploaded under FMH_ROW_HI=2 (tables at any size), FMH_ROW_HI=0 (none) and with the option untouched, through the
host packer, as host bit planes with RANDOM bits under the uncalled entries, as u8 rows (pca_scan_bytes_kernel) and through the device
packer.  Before the device is called every case checks on the reference alone that it is not vacuous: every flag value the kind permits
occurs, every one-flaw row is present at every boundary column inside the row, at least half of the rows are clean (table entry 0).

Gather + Gram: the kept rows are the clean rows of a matrix declared max_allele = 3 with a called plane, between rows with missing calls
and alleles up to 3; the tolerance is tests/test_gpu_pca.py's derived bound, and the Gram must carry the same bits as the Gram of the
kept rows uploaded alone (the same kernel on the same bits).

ferromic.chromosome_pca: 4 500 variants x 40 samples, above the table threshold, with and without the tables.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pca_ref as R
from tests.test_gpu_ld import missing_words, upload
from tests.test_gpu_pca import binary_rows, check_scores, cpu_pair, gram_expectation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


# ---- scan cohorts -------------------------------------------------------------------------------------------------------------------
KINDS = {  # max_allele, missing calls: each plane pointer and each table is present in one kind and absent in another
    "A": (1, True),   # pc, row_gap
    "B": (3, False),  # p1, row_hi
    "C": (7, True),   # p1, p2, pc, both tables
    "D": (1, False),  # neither: every flag 0, the count still checked
}
FLAWS = ("uncalled", "high", "high_uncalled", "one_uncalled")
HIGH_VALUES = {3: (2, 3), 7: (2, 4, 3, 5, 6, 7)}  # 2: plane 1 alone, 4: plane 2 alone
# columns -> ploidy (the scan has no ploidy rule; 4 097 and 8 191 can only be haploid, 8 193 = 3 x 2 731)
PLOIDY = {1: 1, 63: 3, 64: 2, 65: 1, 70: 2, 128: 2, 129: 3, 4095: 3, 4096: 2, 4097: 1, 8191: 1, 8193: 3}
SHAPES = [(c, 300) for c in (1, 63, 64, 65, 128, 129, 4095, 4096, 4097, 8191, 8193)] + [(70, 4100)]  # 4 100 rows: tables by default
TABLES = ("2", "0", None)  # FMH_ROW_HI: tables at any size, none, untouched
ROUTES = ("host", "planes", "bytes", "pack", "pack_release")
SENTINEL_ALT, SENTINEL_FLAG = 0xDEADBEEF, 0xA5


def boundary_columns(cols):
    return sorted({c for c in (0, 1, 31, 32, 63, 64, 127, 128, 4095, 4096, 4097, cols - 65, cols - 64, cols - 1) if 0 <= c < cols})


def flaw_applies(flaw, max_allele, missing):
    return {"uncalled": missing, "one_uncalled": missing, "high": max_allele > 1, "high_uncalled": missing and max_allele > 1}[flaw]


@functools.lru_cache(maxsize=None)
def scan_cohort(kind, cols, rows):
    """x [rows][cols] uint8, called [rows][cols] bool (all True when the kind has no missing calls), the reference counts and flags, and
    marks[(flaw, column)] = the row that carries exactly that flaw.  The special rows are scattered over the matrix."""
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(100_000 * "ABCD".index(kind) + 10 * cols + rows)
    x = (rng.random((rows, cols)) < rng.uniform(0.05, 0.95, size=(rows, 1))).astype(np.uint8)
    called = np.ones((rows, cols), dtype=bool)
    free = list(rng.permutation(rows))
    marks = {}
    for i, c in enumerate(boundary_columns(cols)):
        for flaw in FLAWS:
            if not flaw_applies(flaw, max_allele, missing):
                continue
            r = int(free.pop())
            marks[(flaw, c)] = r
            if flaw in ("high", "high_uncalled"):
                x[r, c] = HIGH_VALUES[max_allele][i % len(HIGH_VALUES[max_allele])]
            if flaw == "one_uncalled":
                x[r, c] = 1
            if flaw != "high":
                called[r, c] = False
    all_one = int(free.pop())
    x[all_one] = 1
    all_uncalled = None
    if missing:
        all_uncalled = int(free.pop())
        called[all_uncalled] = False
    for i in range(rows // 10):  # random flaws: uncalled entries, high alleles, both (on distinct columns)
        r = int(free.pop())
        perm = rng.permutation(cols)
        k = 1 + int(rng.integers(1 + cols // 50))
        want_u, want_h = missing and i % 3 != 1, max_allele > 1 and i % 3 != 0
        u = perm[:k] if want_u else perm[:0]
        h = perm[u.size:u.size + k] if want_h else perm[:0]
        called[r, u] = False
        if h.size:
            x[r, h] = rng.integers(2, max_allele + 1, size=h.size)
    flags = np.where((~called).any(axis=1), 1, 0) | np.where(((x > 1) & called).any(axis=1), 2, 0)
    alt = ((x == 1) & called).sum(axis=1)
    for a in (x, called):
        a.setflags(write=False)
    return SimpleNamespace(kind=kind, cols=cols, rows=rows, max_allele=max_allele, missing=missing, x=x, called=called if missing else None,
                           mask=called, words=missing_words(called) if missing else None, alt=alt.astype(np.uint32), flags=flags.astype(np.uint8),
                           marks=marks, all_one=all_one, all_uncalled=all_uncalled)


def assert_not_vacuous(co):
    """On the reference alone, before the device is called."""
    permitted = {0} | ({1} if co.missing else set()) | ({2} if co.max_allele > 1 else set())
    if co.missing and co.max_allele > 1 and co.cols > 1:
        permitted.add(3)  # uncalled AND a called high allele needs two columns
    assert set(np.unique(co.flags).tolist()) == permitted, (co.kind, co.cols, np.unique(co.flags))
    assert (co.flags == 0).sum() * 2 >= co.rows
    x, called = co.x, co.mask
    for c in boundary_columns(co.cols):
        for flaw in FLAWS:
            if not flaw_applies(flaw, co.max_allele, co.missing):
                continue
            r = co.marks[(flaw, c)]
            uncalled, high = np.nonzero(~called[r])[0], np.nonzero(x[r] > 1)[0]
            if flaw == "uncalled":
                assert uncalled.tolist() == [c] and high.size == 0 and co.flags[r] == 1
            elif flaw == "high":
                assert uncalled.size == 0 and high.tolist() == [c] and co.flags[r] == 2 and co.alt[r] == (x[r] == 1).sum()
            elif flaw == "high_uncalled":
                assert uncalled.tolist() == [c] and high.tolist() == [c] and co.flags[r] == 1
            else:
                assert uncalled.tolist() == [c] and high.size == 0 and x[r, c] == 1 and co.flags[r] == 1 and co.alt[r] == (x[r] == 1).sum() - 1
    assert co.alt[co.all_one] == co.cols and co.flags[co.all_one] == 0
    if co.missing:
        assert co.alt[co.all_uncalled] == 0 and co.flags[co.all_uncalled] == 1
    if co.kind == "C":
        assert {int(co.x[co.marks[("high", c)], c]) for c in boundary_columns(co.cols)} >= ({2, 4} if co.cols >= 2 else {2})


def open_route(dev, fmh_opts, co, route):
    """The cohort as a device matrix that the scan reads through `route`.  FMH_ROW_HI is the caller's: the uploads and fmh_matrix_pack
    read it when they build (or do not build) the tables."""
    rows, cols, ploidy = co.rows, co.cols, PLOIDY[co.cols]
    if route == "planes":  # random bits under the uncalled entries of every allele plane, padding bits zero
        # (upload() declares ploidy 2 for an even column count, else 1, whatever PLOIDY says: ploidy 3 meets the other four routes)
        fmh_opts.setenv("FMH_LAYOUT", "packed")
        return upload(dev, co.x, co.called, co.max_allele, planes=True, seed=cols)
    fmh_opts.setenv("FMH_LAYOUT", "packed" if route == "host" else "bytes")
    # the bytes as they are: alleles 1 and above stay under the uncalled entries
    dm = dev.DeviceMatrix.from_host(co.x, co.words, rows, cols // ploidy, ploidy, co.max_allele)
    if route in ("pack", "pack_release"):
        try:
            dm.pack(release_bytes=route == "pack_release")
        except Exception:
            dm.close()
            raise
        fmh_opts.setenv("FMH_LAYOUT", "packed")  # beside the u8 rows the packed image is scanned only when bytes are not forced
    return dm


def set_tables(fmh_opts, tables):
    if tables is None:
        fmh_opts.delenv("FMH_ROW_HI")
    else:
        fmh_opts.setenv("FMH_ROW_HI", tables)


def first_differences(got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(r), int(got[r]), int(want[r])) for r in bad[:6]]


@pytest.mark.parametrize("cols,rows", SHAPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_scan_equals_numpy_on_every_route_with_and_without_tables(dev, fmh_opts, kind, cols, rows):
    co = scan_cohort(kind, cols, rows)
    assert_not_vacuous(co)
    seen = []
    for tables in TABLES:
        set_tables(fmh_opts, tables)
        for route in ROUTES:
            dm = open_route(dev, fmh_opts, co, route)
            try:
                assert (dm.variants, dm.columns) == (rows, cols)
                alt, flags = dev.pca_scan_sites(dm)
            finally:
                dm.close()
            what = (kind, cols, rows, f"FMH_ROW_HI={tables}", route)
            assert np.array_equal(flags, co.flags), (what, "flags (row, got, expected)", first_differences(flags, co.flags))
            assert np.array_equal(alt, co.alt), (what, "alt (row, got, expected)", first_differences(alt, co.alt))
            seen.append((alt, flags))
    assert all(np.array_equal(a, seen[0][0]) and np.array_equal(f, seen[0][1]) for a, f in seen)


def scan_into_sentinels(dev, dm, row_begin, row_count, pad=9):
    """fmh_pca_scan_sites into buffers of row_count + pad entries filled with sentinels; returns them whole.  (dev.pca_scan_sites
    allocates its outputs itself, exactly row_count entries and uninitialised, so it can show neither a write beyond row_count nor that
    an empty range wrote nothing: this goes to the C call with buffers of its own.)"""
    from ferromic_amd import _abi

    d_alt = dev.DeviceBuffer.from_numpy(dm.device, np.full(row_count + pad, SENTINEL_ALT, dtype=np.uint32))
    d_flags = dev.DeviceBuffer.from_numpy(dm.device, np.full(row_count + pad, SENTINEL_FLAG, dtype=np.uint8))
    _abi.check(_abi.load().fmh_pca_scan_sites(dm._h, row_begin, row_count, d_alt.ptr, d_flags.ptr, None))
    return d_alt.to_numpy(np.uint32, row_count + pad), d_flags.to_numpy(np.uint8, row_count + pad)


@pytest.mark.parametrize("cols", [129, 4097])
@pytest.mark.parametrize("kind", ["A", "B", "C"])
def test_scan_row_ranges_on_a_matrix_with_tables(dev, fmh_opts, kind, cols):
    """The tables are indexed by the absolute row, the outputs by the relative one; entries beyond row_count stay as they were, and the
    empty range writes nothing."""
    from ferromic_amd import _abi

    S = 300
    co = scan_cohort(kind, cols, S)
    assert_not_vacuous(co)
    ranges = [(0, S), (1, S - 2), (5, 1), (S - 3, 3), (6, 51), (S, 0)]
    assert ranges[4][0] % 4 != 0 and ranges[4][1] > 8  # begins inside a 4-row block of the launch, spans more than one
    # indexed by the relative row a table would hide a flaw: some row of the range needs a plane while the byte `begin` rows before it is 0
    # (row_gap: no uncalled entry; row_hi: no bit above plane 0 on any route - no allele above 1 and nothing uncalled to hold random bits)
    gap_zero, hi_zero = (co.flags & 1) == 0, ~(co.x > 1).any(axis=1) & co.mask.all(axis=1)
    for begin, count in ((1, S - 2), (6, 51)):
        needs = co.flags[begin:begin + count]
        assert not co.missing or ((needs & 1 != 0) & gap_zero[:count]).any(), (begin, count, "row_gap")
        assert co.max_allele == 1 or ((needs & 2 != 0) & hi_zero[:count]).any(), (begin, count, "row_hi")
    fmh_opts.setenv("FMH_ROW_HI", "2")
    for route in ROUTES:
        dm = open_route(dev, fmh_opts, co, route)
        try:
            for begin, count in ranges:
                alt, flags = scan_into_sentinels(dev, dm, begin, count)
                what = (kind, cols, route, begin, count)
                assert np.array_equal(flags[:count], co.flags[begin:begin + count]), (what, first_differences(flags[:count], co.flags[begin:begin + count]))
                assert np.array_equal(alt[:count], co.alt[begin:begin + count]), (what, first_differences(alt[:count], co.alt[begin:begin + count]))
                assert np.all(alt[count:] == SENTINEL_ALT) and np.all(flags[count:] == SENTINEL_FLAG), (what, "written beyond row_count")
            alt, flags = dev.pca_scan_sites(dm, 7)  # the wrapper's default count
            assert np.array_equal(alt, co.alt[7:]) and np.array_equal(flags, co.flags[7:])
            for begin, count in ((S + 1, 0), (S - 1, 2)):
                with pytest.raises(_abi.FerromicHipError, match="exceed"):
                    dev.pca_scan_sites(dm, begin, count)
        finally:
            dm.close()


# ---- the gather and the Gram on a mixed matrix --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_cohort(n, m):
    """rows x n, max_allele 3 with missing calls: m clean rows (the kept set: row 0, the last row, holes everywhere) between rows that carry
    uncalled entries and alleles 2 and 3.  Returns the cohort and the expectation of tests/test_gpu_pca.py for the kept rows."""
    rng = np.random.default_rng(7000 * n + m)
    rows = m + m // 3 + 5
    kept = np.sort(np.concatenate(([0, rows - 1], rng.choice(np.arange(1, rows - 1), size=m - 2, replace=False)))).astype(np.uint64)
    dirty = np.setdiff1d(np.arange(rows), kept.astype(np.int64))
    x = binary_rows(rng, rows, n)
    called = np.ones((rows, n), dtype=bool)
    called[dirty] = rng.random((dirty.size, n)) >= 0.05
    called[dirty, rng.integers(n, size=dirty.size)] = False
    xd = x[dirty]
    high = (xd == 1) & (rng.random(xd.shape) < 0.3)
    xd[high] = rng.integers(2, 4, size=int(high.sum()))
    xd[np.arange(dirty.size), rng.integers(n, size=dirty.size)] = 2 + np.arange(dirty.size) % 2
    x[dirty] = xd
    for a in (x, called):
        a.setflags(write=False)
    hi, lo, _, expected, bound = gram_expectation(x[kept.astype(np.int64)], n)
    return SimpleNamespace(n=n, m=m, rows=rows, x=x, called=called, words=missing_words(called), kept=kept, dirty=dirty, hi=hi, lo=lo,
                           expected=expected, bound=bound)


def assert_mixed_not_vacuous(co):
    """The kept rows are exactly the clean ones, first and last row among them, and dirty rows sit between kept rows."""
    ki, m = co.kept.astype(np.int64), co.m
    assert ki[0] == 0 and ki[-1] == co.rows - 1 and co.kept.size == m
    assert co.called[ki].all() and co.x[ki].max() == 1
    assert (~co.called[co.dirty]).any(axis=1).all() and ((co.x[co.dirty] > 1) & co.called[co.dirty]).any(axis=1).all()
    assert {2, 3} <= set(np.unique(co.x[co.dirty]).tolist())
    assert np.isin(ki[1:-1] - 1, co.dirty).sum() > m // 8 and np.isin(ki[1:-1] + 1, co.dirty).sum() > m // 8
    return ki


def open_mixed(dev, fmh_opts, co, route):
    if route == "planes":
        fmh_opts.setenv("FMH_LAYOUT", "packed")  # for the clean matrix the caller uploads next
        return upload(dev, co.x, co.called, 3, planes=True, seed=co.m)
    fmh_opts.setenv("FMH_LAYOUT", "packed" if route == "host" else "bytes")
    return dev.DeviceMatrix.from_host(co.x, co.words, co.rows, co.n // 2, 2, 3)


@pytest.mark.parametrize("route", ["host", "planes", "bytes"])
@pytest.mark.parametrize("n,m,splits", [(130, 257, 0), (512, 4097, 3)])
def test_gram_of_the_clean_rows_of_a_mixed_matrix(dev, fmh_opts, n, m, splits, route):
    co = mixed_cohort(n, m)
    ki = assert_mixed_not_vacuous(co)
    fmh_opts.setenv("FMH_ROW_HI", "2")
    if splits:
        fmh_opts.setenv("FMH_PCA_SPLITS", splits)
    dm = open_mixed(dev, fmh_opts, co, route)
    try:
        alt, flags = dev.pca_scan_sites(dm)
        got = dev.pca_gram(dm, co.kept, co.hi, co.lo)
        again = dev.pca_gram(dm, co.kept, co.hi, co.lo)
    finally:
        dm.close()
    # the scan's clean rows are the kept set, and its counts are the ones the standardisation was derived from
    assert np.array_equal(np.nonzero(flags == 0)[0], ki) and np.array_equal(alt[ki], co.x[ki].sum(axis=1))
    err = np.abs(got - co.expected)
    worst = float((err / co.bound).max())
    print(f"mixed gram n={n} m={m} route={route} splits={splits}: max err {err.max():.3e}, max err/bound {worst:.3e}")
    assert np.all(err <= co.bound), (n, m, route, splits, worst)
    assert np.array_equal(got, got.T), "the Gram must be exactly symmetric"
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "two runs on the same input must give the same bits"
    # the kept rows alone, as a clean biallelic matrix in the same layout: the same kernel on the same bits
    alone = dev.DeviceMatrix.from_host(co.x[ki], None, m, n // 2, 2, 1)
    try:
        clean = dev.pca_gram(alone, np.arange(m, dtype=np.uint64), co.hi, co.lo)
    finally:
        alone.close()
    assert np.array_equal(got.view(np.uint64), clean.view(np.uint64)), (n, m, route, float(np.abs(got - clean).max()))


@pytest.mark.parametrize("route", ["host", "planes", "bytes"])
def test_gather_takes_bit_zero_of_the_allele_and_nothing_else(dev, fmh_opts, route):
    """Both gather kernels define a kept row's bit as bit 0 of the entry (plane 0, the low bit of a byte).  The host filter never keeps a row
    with an allele above 1, so only this test can tell whether the upper planes leak into the gathered word: fully called rows with
    alleles 0..3 are gathered, and the Gram must carry the bits of the Gram of (allele & 1) uploaded as a clean matrix."""
    n, m = 130, 257
    rng = np.random.default_rng(31)
    x = rng.integers(0, 4, size=(m, n), dtype=np.uint8)
    low = (x & 1).astype(np.uint8)
    low[:, 0], low[:, n - 1] = 1, 0  # both alleles in every row: a positive variance
    x[:, 0], x[:, n - 1] = 1 + 2 * (np.arange(m) % 2), 2 * (np.arange(m) % 2)
    assert np.array_equal(x & 1, low) and (x >= 2).sum() > x.size // 3 and (low != (x > 0)).any()
    called = np.ones((m, n), dtype=bool)
    called[0, 5] = False  # the matrix has a called plane; row 0 is not gathered
    kept = np.arange(1, m, dtype=np.uint64)
    hi, lo, _, expected, bound = gram_expectation(low[1:], n)
    fmh_opts.setenv("FMH_ROW_HI", "2")
    if route == "planes":
        fmh_opts.setenv("FMH_LAYOUT", "packed")
        dm = upload(dev, x, called, 3, planes=True, seed=3)
    else:
        fmh_opts.setenv("FMH_LAYOUT", "packed" if route == "host" else "bytes")
        dm = dev.DeviceMatrix.from_host(x, missing_words(called), m, n // 2, 2, 3)
    alone = dev.DeviceMatrix.from_host(low[1:], None, m - 1, n // 2, 2, 1)
    try:
        got = dev.pca_gram(dm, kept, hi, lo)
        clean = dev.pca_gram(alone, np.arange(m - 1, dtype=np.uint64), hi, lo)
    finally:
        dm.close()
        alone.close()
    assert np.all(np.abs(got - expected) <= bound), (route, float((np.abs(got - expected) / bound).max()))
    assert np.array_equal(got.view(np.uint64), clean.view(np.uint64)), route


# ---- ferromic.chromosome_pca above the table threshold ----------------------------------------------------------------------------------------
THRESHOLD_SEED = 4500


@functools.lru_cache(maxsize=None)
def threshold_cohort():
    """4 500 variants x 40 samples, three populations (int16): about 300 rows with one missing call, about 250 with one allele from 2 to
    300, a few with both; flaws in the first and the last row."""
    variants, samples = 4500, 40
    g = R.pybench_cohort(variants, samples, seed=THRESHOLD_SEED, scale=0.15, populations=3).astype(np.int16)
    rng = np.random.default_rng(THRESHOLD_SEED + 1)
    missing_rows = np.union1d(rng.choice(variants, size=300, replace=False), [0])
    high_rows = np.union1d(rng.choice(variants, size=250, replace=False), [variants - 1])
    for r in missing_rows:
        g[r, rng.integers(samples), rng.integers(2)] = -1
    for r in high_rows:
        s, side = rng.integers(samples), rng.integers(2)
        while g[r, s, side] < 0:  # a row with both flaws carries them on different entries
            s, side = rng.integers(samples), rng.integers(2)
        g[r, s, side] = rng.integers(2, 300)
    g.setflags(write=False)
    return g, missing_rows, high_rows


@functools.lru_cache(maxsize=None)
def threshold_expectation():
    """The cohort, what the oracle keeps and the conclusive CPU pair - with the checks, on the reference alone, that the case is not vacuous."""
    g, missing_rows, high_rows = threshold_cohort()
    variants, samples = g.shape[:2]
    positions = np.cumsum(np.arange(1, variants + 1, dtype=np.int64))
    names = [f"n{i}" for i in range(samples)]
    flat = g.reshape(variants, 2 * samples)
    flawed = np.union1d(missing_rows, high_rows)
    # not vacuous, on the reference alone: the flaws are where they should be, and most flawed rows would pass the frequency filter
    assert variants >= 4096 and np.array_equal(np.nonzero((flat < 0).any(axis=1))[0], missing_rows)
    assert np.array_equal(np.nonzero((flat > 1).any(axis=1))[0], high_rows) and flat.max() > 255
    assert np.intersect1d(missing_rows, high_rows).size >= 3 and flawed[0] == 0 and flawed[-1] == variants - 1
    freq = np.clip(flat[flawed], 0, 1).sum(axis=1) / float(2 * samples)
    assert (np.minimum(freq, 1 - freq) >= 0.1).sum() > 200  # a flag the scan missed would keep these rows
    _, _, exp_pos = R.chromosome_pca(g, positions, names, 4)
    a, w, d0, kept = cpu_pair(g, 4)
    assert np.array_equal(exp_pos, positions[kept]) and not np.isin(kept, flawed).any() and kept.size > 2000
    return g, positions, names, exp_pos, a, w, d0


def test_chromosome_pca_above_the_table_threshold(fm, fmh_opts):
    g, positions, names, exp_pos, a, w, d0 = threshold_expectation()
    samples = len(names)
    results = []
    for tables in (None, "0"):  # untouched: 4 500 rows get their tables
        set_tables(fmh_opts, tables)
        res = fm.chromosome_pca({"genotypes": g, "positions": positions}, names, 4)
        assert np.array_equal(res.positions, exp_pos), f"FMH_ROW_HI={tables}"
        check_scores(res.coordinates, a, w, d0, 2 * samples, f"4500x40 FMH_ROW_HI={tables}")
        results.append(res.coordinates)
    assert np.array_equal(results[0].view(np.uint64), results[1].view(np.uint64))
