"""Every column-window width, first vector, row range and grid on both routes that read a window: the row-major kernels sized from the window
(sweep_window, enqueue_sweep's lanes per row / batch depth / single trip, row_alt) and the sweep over the tile-transposed plane image
(sweep_tiled_kernels.hpp: HB in {10, 5, 2}, nb = ceil(W / 2 HB) batches, clamped slots of the last batch, tile_base's slot of a lane).
tests/test_gpu_column_window.py and tests/test_gpu_tiled_planes.py hold the hand-picked layouts and the life cycle of the tables; this file fills
in the space between them.

Every case: the C oracle (oracle/dense.py) on the same bytes - counts and integer totals exactly, per-site f64 tracks bit for bit, regional f64
sums to 1e-9; the row-major route without window or image as a second reference for the per-site bits; tiled against row-major at the same
explicit FMH_GRID_BLOCKS for the bits of every regional total; fmh_sweep_window and fmh_sweep_tiled asked for the route and the window, so a
silent fallback fails; and a numpy check (not_vacuous) that the rows swept hold alt bits where a wrong window, clamp or mask would show.

The cohort of (a), (b) and (e): 613 rows (64 * 9 + 37) of 8 190 columns - 64 vectors, two padding bits in the last - whose allele frequency
changes every 64 columns; FMH_GRID_BLOCKS=1: ten tiles over four waves, each walking two or three."""

import functools

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.test_gpu_column_window import (LAYOUTS, S, check_two_groups, check_wc, check_windows, cohort, expected_window, hull, oracle_two_groups,
                                          run_two_groups, same_bits, span, window)
from tests.test_gpu_tiled_planes import assert_route, image_bytes, same_totals

pytestmark = pytest.mark.gpu

ROWS6, COLS6, VECS6 = 64 * 9 + 37, 8190, 64
RANGES6 = ((0, ROWS6), (13, 550))  # the whole matrix; an unaligned start whose tiles straddle two image tiles, ending inside image tile 8
WIDTHS = tuple(range(1, VECS6 + 1))


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture
def opts(fmh_opts):
    fmh_opts.setenv("FMH_COLUMN_WINDOW", "2")
    fmh_opts.setenv("FMH_TILED_PLANES", "2")
    fmh_opts.setenv("FMH_TILED", "1")
    fmh_opts.setenv("FMH_GRID_BLOCKS", "1")
    return fmh_opts


@functools.lru_cache(maxsize=1)
def cohort6():
    """613 x 8 190, biallelic, nothing missing; the population of a column (which of a row's two frequencies it draws from) changes at random
    every 64 columns, so two column sets that differ have different frequencies, not only different bits."""
    rng = np.random.default_rng(613)
    poc = np.repeat(rng.integers(0, 2, size=(COLS6 + 63) // 64, dtype=np.uint8), 64)[:COLS6]
    data, _ = D.generate(ROWS6, COLS6, 8190613, 0, H.thresholds(ROWS6, 613, sigma=0.15), poc, 0, 16)
    data.setflags(write=False)
    return data


def first_vector(W):
    """Deterministic in W: widths = 0 mod 3 start at vector 0, = 1 mod 3 end on the padded last vector, = 2 mod 3 lie strictly inside."""
    if W % 3 == 0:
        return 0
    if W % 3 == 1:
        return VECS6 - W
    return 1 + (5 * W) % (VECS6 - 1 - W)


def sandwich(W, f=None):
    """Group A = columns [128 f + a, 128 (f + W) - b), group B every other column; A starts inside vector f and ends inside vector f + W - 1.
    a = 0 (a vector edge) only where B still has vector 0, b = 0 only where B still has the last vector, so B's hull is the whole row and
    the window is A's.  Odd widths report B first: derived group 0."""
    f = first_vector(W) if f is None else f
    a = 0 if W % 8 == 0 and f > 0 else 1 + (37 * W) % 127
    b = 0 if W % 8 == 4 and f + W < VECS6 else 2 + (53 * W) % 126
    A = span(COLS6, (128 * f + a, min(128 * (f + W) - b, COLS6)))
    masks = np.stack([A, 1 - A]) if W % 2 == 0 else np.stack([1 - A, A])
    return f, masks, (f, W, -1 if W == VECS6 else 1 - W % 2)  # (the whole row: deriving B saves no vector)


def hull_layout(W):
    """Group A a random ~60 % of [128 f + a, mid), group B of [mid, 128 (f + W) - b), the first and last column of the range forced in: both
    groups counted, nothing derived."""
    f = first_vector(W)
    rng = np.random.default_rng(4000 + W)
    lo, hi = 128 * f + (37 * W) % 60, min(128 * (f + W) - 2 - (53 * W) % 59, COLS6)
    mid = lo + max(1, (hi - lo) * (3 + W % 5) // 10)
    member = (rng.random(COLS6) < 0.6).astype(np.uint8)
    member[lo] = member[hi - 1] = 1
    masks = np.stack([member * span(COLS6, (lo, mid)), member * span(COLS6, (mid, hi))])
    return f, masks, (f, W, -1)


def oracle_rows(flat, total_rows, columns, masks, r0, rows):
    """oracle_two_groups for a biallelic matrix of `total_rows` rows with nothing missing."""
    sub = flat.reshape(total_rows, columns)[r0:r0 + rows].reshape(-1)
    off = [np.nonzero(m)[0] for m in masks]
    every = np.arange(columns)
    goc = np.where(masks[0] != 0, 0, np.where(masks[1] != 0, 1, 255)).astype(np.uint8)
    return {"sp": D.region_sweep(sub, None, rows, columns, 1, off[0], off[1], D.FORMULA_SPARSE, D.FORMULA_SPARSE, 16),
            "de": D.region_sweep(sub, None, rows, columns, 1, off[0], off[1], D.FORMULA_DENSE, -1, 16),
            "all": D.region_sweep(sub, None, rows, columns, 1, every, every, D.FORMULA_SPARSE, -1, 16),
            "wc": D.wc_sites(sub, None, rows, columns, goc, 2, 1),
            "dense": D.hudson_sweep(sub, None, rows, columns, off[0], off[1], 16)}


def not_vacuous(sub, masks, win, what):
    """Among the rows swept (`sub`, [rows][columns]): the last vector of the window holds alt bits in member columns of a counted group, the
    vector just outside each end of the window holds alt bits, and a derived group's count is non-zero somewhere - so one vector too many or
    too few, a clamped slot counted, or the wrong group's mask changes a count."""
    first, count, derived = win
    columns = sub.shape[1]
    counted = (np.delete(masks, derived, axis=0) if derived >= 0 else masks).any(axis=0)
    lo, hi = 128 * (first + count - 1), min(128 * (first + count), columns)
    assert sub[:, lo:hi][:, counted[lo:hi]].any(), f"no alt bit in the window's last vector: {what}"
    if first > 0:
        assert sub[:, 128 * (first - 1):128 * first].any(), f"no alt bit before the window: {what}"
    if hi < columns:
        assert sub[:, hi:hi + 128].any(), f"no alt bit behind the window: {what}"
    if derived >= 0:
        assert sub[:, masks[derived] != 0].any(), f"the derived group counts nothing: {what}"


def both_routes(dev, opts, dm, flat, total_rows, masks, win, r0, rows, what, oracle=None, window_off=False):
    """run_two_groups over rows [r0, r0 + rows) on the tiled route and on the row-major route with the same window: the oracle's results on
    either, the same per-site bits and the same bits of every total.  window_off: once more without window or image, per-site bits.  The options
    must hold FMH_TILED=1 and an explicit grid on entry and do so again on return."""
    columns = dm.columns
    image = image_bytes(total_rows, columns)
    g2 = dev.Groups(dm, masks)
    assert win == expected_window(masks, True), what
    not_vacuous(flat.reshape(total_rows, columns)[r0:r0 + rows], masks, win, what)
    exp = oracle(flat, None, columns, 1, masks, r0, rows) if oracle else oracle_rows(flat, total_rows, columns, masks, r0, rows)
    assert_route(dev, dm, masks, True, image)
    assert window(dev, dm, g2, dev.SWEEP_HUDSON) == win, what
    got = run_two_groups(dev, dm, masks, r0, rows)
    check_two_groups(got, exp, True, f"tiled, {what}")
    opts.setenv("FMH_TILED", "0")
    assert_route(dev, dm, masks, False, image)
    assert window(dev, dm, g2, dev.SWEEP_HUDSON) == win, what
    ref = run_two_groups(dev, dm, masks, r0, rows)
    check_two_groups(ref, exp, True, f"row-major, {what}")
    same_bits(got, ref, what)
    same_totals(got, ref, what)
    if window_off:
        opts.setenv("FMH_COLUMN_WINDOW", "0")
        assert window(dev, dm, g2, dev.SWEEP_HUDSON) == (0, (columns + 127) // 128, -1), what
        same_bits(got, run_two_groups(dev, dm, masks, r0, rows), f"no window, {what}")
        opts.setenv("FMH_COLUMN_WINDOW", "2")
    opts.setenv("FMH_TILED", "1")
    return got


def matrix6(dev):
    return dev.DeviceMatrix.from_host(cohort6(), None, ROWS6, COLS6 // 2, 2, 1)


def test_first_vectors_cover_both_ends_and_the_interior():
    """The condition on f of test_every_window_width: of the 64 widths at least 15 start at vector 0, at least 15 hold the padded last vector and at
    least 15 lie strictly inside; every sandwich and hull layout spans exactly (f, W)."""
    fs = {W: first_vector(W) for W in WIDTHS}
    assert all(0 <= f and f + W <= VECS6 for W, f in fs.items())
    assert sum(f == 0 for f in fs.values()) >= 15
    assert sum(f + W == VECS6 for W, f in fs.items()) >= 15
    assert sum(f > 0 and f + W < VECS6 for W, f in fs.items()) >= 15
    derived = set()
    for W in WIDTHS:
        f, masks, win = sandwich(W)
        assert win == expected_window(masks, True) and win[:2] == (f, W) and (masks.sum(axis=0) == 1).all(), W
        derived.add(win[2])
        f, masks, win = hull_layout(W)
        assert win == expected_window(masks, True) == (f, W, -1) and masks[0].any() and masks[1].any() and not (masks[0] & masks[1]).any(), W
    assert derived == {0, 1, -1}


@pytest.mark.parametrize("W", WIDTHS)
def test_every_window_width(dev, opts, W):
    """A window of W vectors at first vector f(W), one group derived (sandwich) and both counted (hull), on the tiled route, on the row-major route
    and without a window; the row range alternates with W."""
    data = cohort6()
    dm = matrix6(dev)
    r0, rows = RANGES6[W % 2]
    for kind, (f, masks, win) in (("sandwich", sandwich(W)), ("hull", hull_layout(W))):
        assert win[:2] == (f, W), kind
        check_windows(dev, dm, masks, win)
        both_routes(dev, opts, dm, data, ROWS6, masks, win, r0, rows, f"{kind} W={W} f={f} rows [{r0}, +{rows})", window_off=True)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 9, 10, 11, 19, 20, 21, 39, 40, 41, 64])
@pytest.mark.parametrize("HB", [2, 5, 10])
def test_forced_tiled_batch(dev, opts, HB, W):
    """FMH_TILED_BATCH: every instantiation of the tiled kernel at widths that give it an all-clamped second half, a half-clamped half and a long
    steady-state loop; the oracle's results, and the bits of the batch the launcher picks itself."""
    data = cohort6()
    dm = matrix6(dev)
    f, masks, win = sandwich(W)
    r0, rows = RANGES6[(W + HB) % 2]
    what = f"HB={HB} W={W} f={f} rows [{r0}, +{rows})"
    assert window(dev, dm, dev.Groups(dm, masks), dev.SWEEP_HUDSON) == win == expected_window(masks, True)
    not_vacuous(data.reshape(ROWS6, COLS6)[r0:r0 + rows], masks, win, what)
    assert_route(dev, dm, masks, True, image_bytes(ROWS6, COLS6))
    unforced = run_two_groups(dev, dm, masks, r0, rows)
    opts.setenv("FMH_TILED_BATCH", str(HB))
    assert_route(dev, dm, masks, True, image_bytes(ROWS6, COLS6))
    got = run_two_groups(dev, dm, masks, r0, rows)
    opts.delenv("FMH_TILED_BATCH")
    check_two_groups(got, oracle_rows(data, ROWS6, COLS6, masks, r0, rows), True, what)
    same_bits(got, unforced, what)
    same_totals(got, unforced, what)


def row_ranges(total):
    """Starts on, just before and just behind image-tile edges with lengths around one and two tiles, and every range that ends with the matrix
    from a start around its last tile edge."""
    tail = total // 64 * 64
    out = [(r0, n) for r0 in (0, 1, 63, 64, 65, 127, tail) for n in (1, 2, 63, 64, 65, 128, 129) if r0 + n <= total]
    return out + [(r0, total - r0) for r0 in (tail - 1, tail, tail + 1, total - 1)]


def test_row_ranges_on_the_tiled_route(dev, opts):
    """tile_base: a lane's slot in the image for ranges that start on, before and behind a tile edge, shorter than a tile across two image tiles,
    one row, and ending on the partial last image tile; layout 5000_a_b at 4 517 rows and an interior sandwich at 613 x 8 190."""
    columns, masks, win = LAYOUTS["5000_a_b"]
    data, _ = cohort(columns, "5000_a_b", 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    ranges = row_ranges(S)
    assert (4480, 2) in ranges and (4480, 37) in ranges and (S - 1, 1) in ranges and (4480, 63) not in ranges and len(ranges) == 48
    for r0, rows in ranges:
        both_routes(dev, opts, dm, data, S, masks, win, r0, rows, f"5000_a_b rows [{r0}, +{rows})", oracle=oracle_two_groups)
    f, masks, win = sandwich(11, 37)  # (a position at which even the one-row ranges - row 1 has an allele frequency of 0.09 - pass not_vacuous)
    assert win == (37, 11, 0)
    data = cohort6()
    dm = matrix6(dev)
    for r0, rows in row_ranges(ROWS6):
        both_routes(dev, opts, dm, data, ROWS6, masks, win, r0, rows, f"sandwich W=11 f=37 rows [{r0}, +{rows})")


@pytest.mark.parametrize("key", ["5000_a_b", "5000_no_partition"])
def test_grids(dev, opts, key):
    """One, three and seven workgroups (a wave's tiles are 4, 12 and 28 apart): the oracle's results and, at each grid, the bits of every total
    equal between the routes.  The default grid: the oracle's results on either route (the routes may choose different grids)."""
    columns, masks, win = LAYOUTS[key]
    data, _ = cohort(columns, key, 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    r0, rows = 13, 3000
    for blocks in (1, 3, 7):
        opts.setenv("FMH_GRID_BLOCKS", str(blocks))
        both_routes(dev, opts, dm, data, S, masks, win, 0, S, f"{key}, {blocks} blocks", oracle=oracle_two_groups)
        both_routes(dev, opts, dm, data, S, masks, win, r0, rows, f"{key}, {blocks} blocks, rows [{r0}, +{rows})", oracle=oracle_two_groups)
    opts.delenv("FMH_GRID_BLOCKS")
    exp = oracle_two_groups(data, None, columns, 1, masks, 0, S)
    for tiled in (True, False):
        opts.setenv("FMH_TILED", "1" if tiled else "0")
        assert_route(dev, dm, masks, tiled, image_bytes(S, columns))
        assert window(dev, dm, dev.Groups(dm, masks), dev.SWEEP_HUDSON) == win
        check_two_groups(run_two_groups(dev, dm, masks, 0, S), exp, True, f"{key}, default grid, tiled={tiled}")


def contiguous_groups(G, W):
    """G contiguous groups of unequal sizes that fill [128 f + a, 128 (f + W) - b): their hull is (f, W); f > 0 where W < 64."""
    f = 0 if W == VECS6 else 1 + (3 * W + G) % (VECS6 - W)
    lo, hi = 128 * f + (11 * W + G) % 32, min(128 * (f + W) - 2 - (7 * W + G) % 30, COLS6)
    cum = np.concatenate([[0], np.cumsum(np.arange(1, G + 1))])
    edges = lo + (hi - lo) * cum // cum[-1]
    assert (np.diff(edges) > 0).all()
    return f, np.stack([span(COLS6, (int(edges[k]), int(edges[k + 1]))) for k in range(G)])


@pytest.mark.parametrize("W", [1, 3, 12, 13, 20, 21, 32, 33, 48, 64])
@pytest.mark.parametrize("G", [3, 4, 5, 8])
def test_wc_and_summaries_of_many_groups_read_their_hull(dev, opts, G, W):
    """W&C and the summaries of three to eight contiguous groups read the hull of the groups on their own routes - lanes per row, batch depth and
    the shallow set of five and more groups sized from the window - never the image, never a derived group."""
    data = cohort6()
    dm = matrix6(dev)
    f, masks = contiguous_groups(G, W)
    goc = np.full(COLS6, 255, dtype=np.uint8)
    for k in range(G):
        goc[masks[k] != 0] = k
    g = dev.Groups(dm, masks)
    win = (f, W, -1)
    assert (*hull(masks), -1) == win and (W == VECS6 or f > 0)
    for r0, rows in RANGES6:
        what = f"G={G} W={W} f={f} rows [{r0}, +{rows})"
        sub = data.reshape(ROWS6, COLS6)[r0:r0 + rows]
        not_vacuous(sub, masks, win, what)
        for mode in (dev.SWEEP_WC, dev.SWEEP_SUMMARY):
            assert window(dev, dm, g, mode) == win, (mode, what)
            assert dev.sweep_tiled(dm, g, mode) == (False, image_bytes(ROWS6, COLS6)), (mode, what)
        got = dev.wc_sweep(dm, g, r0, rows)
        check_wc(got, D.wc_sites(sub.reshape(-1), None, rows, COLS6, goc, G, 1), what)
        ps = dev.population_summaries(dm, g, dev.FORMULA_SPARSE, r0, rows)
        assert np.array_equal(ps.alt, np.stack([sub[:, masks[k] != 0].sum(axis=1, dtype=np.uint32) for k in range(G)])), what
        assert np.array_equal(ps.called, np.repeat(masks.sum(axis=1, dtype=np.uint32)[:, None], rows, axis=1)), what
        opts.setenv("FMH_COLUMN_WINDOW", "0")
        assert window(dev, dm, g, dev.SWEEP_WC) == (0, VECS6, -1) and window(dev, dm, g, dev.SWEEP_SUMMARY) == (0, VECS6, -1)
        off = dev.wc_sweep(dm, g, r0, rows)
        ps0 = dev.population_summaries(dm, g, dev.FORMULA_SPARSE, r0, rows)
        opts.setenv("FMH_COLUMN_WINDOW", "2")
        for k in range(got.a.shape[0]):
            H.assert_bits_equal(got.a[k], off.a[k], f"W&C a {k} {what}")
            H.assert_bits_equal(got.b[k], off.b[k], f"W&C b {k} {what}")
        assert np.array_equal(got.state, off.state) and np.array_equal(ps.alt, ps0.alt), what
