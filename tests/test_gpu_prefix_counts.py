"""The prefix counts of plane 0 (fmh_matrix's p0c, FMH_PREFIX_COUNTS) and the table form of the tiled sweep (sweep_kernel_tiled_prefix):
a counted group whose members are one column range is the difference of two table entries plus the masked counts of its at most two
partial edge vectors; the whole vectors of the range are not read.

Every case compares with the C oracle (oracle/dense.py) on the same bytes, exactly as tests/test_gpu_tiled_planes.py does (counts and
integer totals exactly, per-site f64 tracks bit for bit, regional f64 sums to 1e-9), and with the same sweeps under FMH_PREFIX_COUNTS=0 (the
window of the tiled route, the table still present): per-site tracks AND regional sums bit for bit - the same grid, the same order of every
sum; the whole row range is compared with FMH_TILED=0 in the same way.  Every case asks fmh_sweep_prefix whether the sweep takes the table
form and how many vectors it still reads, and the test works both out from the masks alone, so a case that silently fell back does not count.

Shapes: rows of 1, 2, 3 and 40 vectors (122, 250, 384 and 5 000 columns: a masked tail in the last vector, and none) at 63, 64, 65 and 130
rows - less than an image tile, exactly one, one row more, and three tiles with a partial one; the whole matrix and a row range that starts
at row 5 or 13, so that every 64-row tile of the sweep straddles two image tiles; grids of 1 and 3 workgroups.  FMH_TILED_PLANES=2,
FMH_PREFIX_COUNTS=2 and FMH_COLUMN_WINDOW=2 build the image, the table and the row totals at these sizes, FMH_TILED=1 takes the tiled route
wherever it is built."""

import struct

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.test_gpu_column_window import check_two_groups, run_two_groups, same_bits, span
from tests.test_gpu_scale_sparse import TRACKS
from tests.test_gpu_tiled_planes import oracle_whole_matrix, same_totals

pytestmark = pytest.mark.gpu

COLUMNS = {1: 122, 2: 250, 3: 384, 40: 5000}
ROWS = (63, 64, 65, 130)


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture
def prefix_opts(fmh_opts):
    fmh_opts.setenv("FMH_TILED_PLANES", "2")
    fmh_opts.setenv("FMH_PREFIX_COUNTS", "2")
    fmh_opts.setenv("FMH_COLUMN_WINDOW", "2")
    fmh_opts.setenv("FMH_TILED", "1")
    fmh_opts.setenv("FMH_GRID_BLOCKS", "1")
    return fmh_opts


def table_bytes(rows, columns):
    return (rows + 63) // 64 * ((columns + 127) // 128 + 1) * 128


def layouts(vectors, columns):
    """name -> two masks.  Ranges that start or end on a vector boundary, one column to either side of it, inside a single vector, across the
    whole row, and without a whole vector between their edges; partitions (one group derived) and pairs with a gap (both counted); one group
    that is not a range."""
    c = columns
    out = {"halves": [[(0, c // 2)], [(c // 2, c)]],                 # a partition: the second group is derived
           "halves swapped": [[(c // 2, c)], [(0, c // 2)]],
           "inside one vector": [[(3, 40)], [(41, min(c, 128) - 1)]],  # both counted, no whole vector in either
           "first column | rest": [[(0, 1)], [(1, c)]],
           "row but the last column | it": [[(0, c - 1)], [(c - 1, c)]],
           "not a range": [[(0, 10), (20, 30)], [(40, c)]]}
    if vectors >= 2:
        out["cut on a boundary"] = [[(0, 128)], [(128, c)]]
        out["cut one column past it"] = [[(0, 129)], [(129, c)]]
        out["cut one column before it"] = [[(0, 127)], [(127, c)]]
        out["two partial vectors, nothing whole"] = [[(100, 200)], [(201, c - 2)]]
        out["whole vector | gap | rest"] = [[(0, 128)], [(130, c)]]
    if vectors >= 3:
        out["middle vector alone"] = [[(128, 256)], [(0, 128), (256, c)]]  # the counted group: whole vectors only; the derived one is no range
        out["starts on a boundary, ends inside"] = [[(128, 300)], [(301, c)]]
        out["starts inside, ends on a boundary"] = [[(5, 256)], [(260, c - 3)]]
    if vectors == 40:
        out["the benchmark's split"] = [[(0, 2500)], [(2500, c)]]
        out["two inner ranges"] = [[(300, 900)], [(3000, 3700)]]
        out["cut at 2560"] = [[(0, 2560)], [(2560, c)]]
    return {k: np.stack([span(c, *g) for g in v]) for k, v in out.items()}


def ranges_of(mask):
    cols = np.nonzero(mask)[0]
    return None if cols.size == 0 or cols[-1] - cols[0] + 1 != cols.size else (int(cols[0]), int(cols[-1]) + 1)


def partial_vectors(c0, c1, columns):
    n = 0
    for v in range(c0 // 128, (c1 - 1) // 128 + 1):
        lo, hi = 128 * v, min(128 * v + 128, columns)
        inside = min(c1, hi) - max(c0, lo)
        n += 0 < inside < hi - lo
    return n


def expected_route(dev, dm, g, masks, mode):
    """(table form?, vectors read) from the masks and the window alone: every counted group one range -> its partial vectors."""
    first, count, derived = dev.sweep_window(dm, g, mode)
    counted = [ranges_of(masks[p]) for p in range(masks.shape[0]) if p != derived]
    if not counted or any(r is None for r in counted):
        return False, count
    return True, sum(partial_vectors(r[0], r[1], dm.columns) for r in counted)


def assert_routes(dev, dm, masks, table, on=True):
    g2 = dev.Groups(dm, masks)
    some = False
    for g, m, mode in [(g2, masks, md) for md in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION)] + \
                      [(dev.Groups(dm, masks[p:p + 1]), masks[p:p + 1], dev.SWEEP_DIVERSITY) for p in range(2)]:
        uses, vecs = expected_route(dev, dm, g, m, mode)
        if not on:
            uses, vecs = False, dev.sweep_window(dm, g, mode)[1]
        assert dev.sweep_prefix(dm, g, mode) == (uses, vecs, table), (mode, dev.sweep_prefix(dm, g, mode), uses, vecs)
        some = some or uses
    assert dev.sweep_prefix(dm, g2, dev.SWEEP_WC)[0] is False
    return some


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("vectors", sorted(COLUMNS))
def test_table_form_against_the_window_and_the_oracle(dev, prefix_opts, vectors, rows):
    columns = COLUMNS[vectors]
    table = table_bytes(rows, columns)
    r0 = 13 if rows > 65 else 5
    for name, masks in layouts(vectors, columns).items():
        data, _ = D.generate(rows, columns, 100 + vectors, 0, H.thresholds(rows, 7), masks[1].astype(np.uint8), 0, 16)
        dm = dev.DeviceMatrix.from_host(data, None, rows, columns // 2, 2, 1)
        assert dev.sweep_tiled(dm, dev.Groups(dm, masks), dev.SWEEP_HUDSON)[0] is True, name
        used = assert_routes(dev, dm, masks, table)
        g2 = dev.Groups(dm, masks)
        if name == "not a range":  # the counted group of the Hudson sweep is the split one: the old route; the second group alone is a range
            assert dev.sweep_prefix(dm, g2, dev.SWEEP_HUDSON)[0] is False
            assert dev.sweep_prefix(dm, dev.Groups(dm, masks[1:2]), dev.SWEEP_DIVERSITY)[0] is True
        else:
            assert used and dev.sweep_prefix(dm, g2, dev.SWEEP_HUDSON)[0] is True, name
        for a, n in ((0, rows), (r0, rows - r0 - 2)):
            exp = oracle_whole_matrix(data.reshape(rows, columns)[a:a + n].reshape(-1), n, columns, masks)
            for grid in ("1", "3"):
                what = f"{vectors} vectors, {rows} rows, {name}, rows [{a}, +{n}), grid {grid}"
                prefix_opts.setenv("FMH_GRID_BLOCKS", grid)
                got = run_two_groups(dev, dm, masks, a, n)
                check_two_groups(got, exp, True, what)
                prefix_opts.setenv("FMH_PREFIX_COUNTS", "0")  # read at every sweep: the window, with the table still present
                assert_routes(dev, dm, masks, table, on=False)
                ref = run_two_groups(dev, dm, masks, a, n)
                prefix_opts.setenv("FMH_PREFIX_COUNTS", "2")
                same_bits(got, ref, what)
                same_totals(got, ref, what)
                if a == 0 and grid == "1":
                    prefix_opts.setenv("FMH_TILED", "0")
                    ref = run_two_groups(dev, dm, masks, a, n)
                    prefix_opts.setenv("FMH_TILED", "1")
                    same_bits(got, ref, what + " against the row-major route")
                    same_totals(got, ref, what + " against the row-major route")


def bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def test_table_follows_every_pack(dev, prefix_opts):
    """Generate, pack, sweep; generate with another seed, pack, sweep: the second sweep is the second cohort's, so a stale table would fail.
    A pack with FMH_PREFIX_COUNTS=0 drops the table and one with FMH_TILED_PLANES=0 drops it with the image; the default policy keeps
    matrices below 4 096 rows without one."""
    rows, columns = 130, 5000
    masks = np.stack([span(columns, (0, 2500)), span(columns, (2500, columns))])
    poc = masks[1].astype(np.uint8)
    off = [np.nonzero(m)[0] for m in masks]
    dm = dev.DeviceMatrix.alloc(rows, columns // 2, 2, with_missing=False)
    g = dev.Groups(dm, masks)
    table = table_bytes(rows, columns)

    def check(exp, what):
        got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
        assert np.array_equal(got.sites["alt"], exp.alt), what
        for k in TRACKS:
            H.assert_bits_equal(got.sites[k], getattr(exp, k), f"{k} {what}")
        return got

    for seed in (11, 12):
        thr = H.thresholds(rows, seed)
        dm.generate(seed, 0, thr, poc, 0)
        dm.pack(release_bytes=False)
        assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON) == (True, 1, table)
        hdata, _ = D.generate(rows, columns, seed, 0, thr, poc, 0, 16)
        exp = D.hudson_sweep(hdata, None, rows, columns, off[0], off[1], 16)
        with_table = check(exp, f"seed {seed}")
    prefix_opts.setenv("FMH_PREFIX_COUNTS", "0")
    dm.pack(release_bytes=False)
    prefix_opts.setenv("FMH_PREFIX_COUNTS", "2")  # sweeps would read a table again - but the last pack kept none
    assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON) == (False, 20, 0)
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON)[0] is True
    plain = check(exp, "no table")
    assert {k: bits(v) for k, v in plain.totals.items()} == {k: bits(v) for k, v in with_table.totals.items()}
    dm.pack(release_bytes=False)
    assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON) == (True, 1, table)
    prefix_opts.setenv("FMH_TILED_PLANES", "0")
    dm.pack(release_bytes=False)
    assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON) == (False, 20, 0) and dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (False, 0)
    check(exp, "no image")
    prefix_opts.setenv("FMH_TILED_PLANES", "2")
    prefix_opts.setenv("FMH_PREFIX_COUNTS", "1")  # the default policy: 130 rows are too few
    dm.pack(release_bytes=False)
    assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON) == (False, 20, 0) and dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON)[0] is True
    check(exp, "default policy, small matrix")


@pytest.mark.parametrize("kind", ["missing", "max_allele_2"])
def test_no_table_on_missing_calls_and_on_multi_allelic_rows(dev, prefix_opts, kind):
    rows, columns = 130, 5000
    masks = np.stack([span(columns, (0, 2500)), span(columns, (2500, columns))])
    off = [np.nonzero(m)[0] for m in masks]
    if kind == "missing":
        data, words = D.generate(rows, columns, 3, 0, H.thresholds(rows, 3), masks[1].astype(np.uint8), int(0.01 * (1 << 24)), 16)  # 1 % missing calls
        declared = 1
    else:
        data, words = D.generate(rows, columns, 3, 0, H.thresholds(rows, 3), masks[1].astype(np.uint8), 0, 16)
        data = data.copy()
        data[0] = 2
        data[77 * columns + 2499] = 2
        declared = 2
    dm = dev.DeviceMatrix.from_host(data, words, rows, columns // 2, 2, declared)
    g = dev.Groups(dm, masks)
    assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON)[0] is False and dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON)[2] == 0
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (False, 0)
    got = dev.hudson_sweep(dm, g, dev.FORMULA_SPARSE)
    exp = D.region_sweep(data, words, rows, columns, declared, off[0], off[1], D.FORMULA_SPARSE, D.FORMULA_SPARSE, 16)
    assert np.array_equal(got.sites["called"], exp.called)
    if declared <= 1:
        assert np.array_equal(got.sites["alt"], exp.alt)
    H.assert_bits_equal(got.sites["fst"], exp.fst, kind)


def test_no_table_beyond_u16_columns(dev, prefix_opts):
    """65 536 columns: a count may not fit a u16 entry - the image is built, the table is not, the sweep reads its window; 65 534 columns
    (the widest even row that fits) get the table, and a row of all ones counts 65 534 without wrapping."""
    rows = 65
    for columns, has_table in ((65536, False), (65534, True)):
        masks = np.stack([span(columns, (0, 40000)), span(columns, (40000, columns))])
        off = [np.nonzero(m)[0] for m in masks]
        data, _ = D.generate(rows, columns, 9, 0, H.thresholds(rows, 9), masks[1].astype(np.uint8), 0, 16)
        data = data.copy()
        data[:columns] = 1  # row 0: every column set
        dm = dev.DeviceMatrix.from_host(data, None, rows, columns // 2, 2, 1)
        g = dev.Groups(dm, masks)
        assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON)[0] is True
        uses, vecs, table = dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON)
        assert (uses, table) == (has_table, table_bytes(rows, columns) if has_table else 0), columns
        assert vecs == (1 if has_table else dev.sweep_window(dm, g, dev.SWEEP_HUDSON)[1])
        got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
        exp = D.hudson_sweep(data, None, rows, columns, off[0], off[1], 16)
        assert np.array_equal(got.sites["alt"], exp.alt), columns
        assert got.sites["alt"][0][0] == 40000 and got.sites["alt"][1][0] == columns - 40000
        for k in TRACKS:
            H.assert_bits_equal(got.sites[k], getattr(exp, k), f"{k} at {columns} columns")
        # one group alone, to the row's end: the last boundary's entry is the row total
        g1 = dev.Groups(dm, masks[1:2])
        dv = dev.diversity_sites(dm, g1, 0, rows)
        assert dev.sweep_prefix(dm, g1, dev.SWEEP_DIVERSITY)[0] is has_table
        e1 = D.region_sweep(data, None, rows, columns, 1, off[1], off[1], D.FORMULA_SPARSE, -1, 16)
        H.assert_bits_equal(dv.pi, e1.site_pi[0], f"pi at {columns} columns")
