"""The tile-transposed image of plane 0 (fmh_matrix's p0t, FMH_TILED_PLANES) and the sweeps that read their column window from it
(sweep_tiled_kernels.hpp): lane L owns row L of a 64-row tile, one coalesced 16-byte-per-lane load per window vector, a derived group is
not counted at all.

Every case compares with the C oracle (oracle/dense.py) on the same bytes: counts and integer totals exactly, per-site f64 tracks bit for
bit, regional f64 sums to 1e-9; the same sweeps with FMH_TILED=0 (the row-major routes, the image still present) are a second reference:
per-site tracks AND regional sums bit for bit - the same grid, the same order of every sum.  Every case asks fmh_sweep_tiled whether the
sweep takes the tiled route, so a case that silently fell back does not count.

All cases: 64 * 70 + 37 rows, FMH_TILED_PLANES=2 (the image at any size), FMH_TILED=1 (the route wherever it is built: by
default only a window of at most seven eighths of the row takes it), FMH_COLUMN_WINDOW=2, FMH_GRID_BLOCKS=1, and a second sweep over
rows [13, 13 + 3 000), whose 64-row tiles straddle two image tiles each.

These are hand-picked layouts; tests/test_gpu_window_geometry.py covers every window width 1 .. 64, every FMH_TILED_BATCH, first vectors on both
ends and inside, row ranges that start and end around image-tile edges and grids of 1, 3 and 7 workgroups on this route."""

import ctypes as C
import struct

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.test_gpu_column_window import (LAYOUTS, RANGES, S, check_two_groups, cohort, oracle_two_groups, run_two_groups, same_bits, span,
                                          window)
from tests.test_gpu_scale_sparse import TRACKS, check_pop

pytestmark = pytest.mark.gpu

# (4224_2048_2176: a 16-vector window - the 20-vector batch with its last four slots clamped against a zero mask)
KEYS = ("5000_a_b", "5000_b_a", "5000_4000_1000", "130_1_129", "130_129_1", "512_256_256", "4224_2048_2176", "12000_6000_6000",
        "5000_no_partition", "5000_interleaved")


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture
def tiled_opts(fmh_opts):
    fmh_opts.setenv("FMH_TILED_PLANES", "2")
    fmh_opts.setenv("FMH_TILED", "1")  # wherever the route is built: by default a window of more than seven eighths of the row keeps the row-major route
    fmh_opts.setenv("FMH_COLUMN_WINDOW", "2")
    fmh_opts.setenv("FMH_GRID_BLOCKS", "1")
    return fmh_opts


def image_bytes(rows, columns):
    return (rows + 63) // 64 * ((columns + 127) // 128) * 1024


def sweeps_of(dev, dm, masks):
    """(groups, mode) of every sweep run_two_groups makes that the tiled route covers."""
    g2 = dev.Groups(dm, masks)
    out = [(g2, mode) for mode in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION)]
    out += [(dev.Groups(dm, masks[p:p + 1]), dev.SWEEP_DIVERSITY) for p in range(2)]
    gall = dev.Groups(dm, np.ones((1, dm.columns), dtype=np.uint8))
    return out + [(gall, dev.SWEEP_SUMMARY), (gall, dev.SWEEP_DIVERSITY)]


def assert_route(dev, dm, masks, tiled, image):
    for g, mode in sweeps_of(dev, dm, masks):
        assert dev.sweep_tiled(dm, g, mode) == (tiled, image), mode
    assert dev.sweep_tiled(dm, dev.Groups(dm, masks), dev.SWEEP_WC) == (False, image)  # W&C stays on its routes


def bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def totals_of(got):
    """Every regional total of a run_two_groups result, floats as their bytes."""
    out = {}
    for key in ("dense", "sparse"):
        out[key] = {k: bits(v) for k, v in got[key].totals.items()}
        for p in range(2):
            out[key, p] = {k: bits(v) for k, v in got[key].pop[p].items()}
    for f, fu in got["fused"].items():
        out["fused", f] = {k: bits(v) for k, v in fu["totals"].items()}
        for p in range(2):
            out["fused", f, p] = {k: bits(v) for k, v in fu["pop"][p].items()}
    for p in range(2):
        out["div", p] = {k: bits(v) for k, v in got["div"][p].totals.items()}
        out["ps", p] = {k: bits(v) for k, v in got["ps"].totals[p].items()}
    out["all"] = {k: bits(v) for k, v in got["all"].totals[0].items()}
    out["alldiv"] = {k: bits(v) for k, v in got["alldiv"].totals.items()}
    return out


def same_totals(a, b, what):
    ta, tb = totals_of(a), totals_of(b)
    assert ta.keys() == tb.keys(), what
    for key in ta:
        assert ta[key] == tb[key], (key, what)


@pytest.mark.parametrize("key", KEYS)
def test_two_group_layouts(dev, tiled_opts, key):
    columns, masks, hudson_window = LAYOUTS[key]
    data, _ = cohort(columns, key, 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    image = image_bytes(S, columns)
    g2 = dev.Groups(dm, masks)
    assert window(dev, dm, g2, dev.SWEEP_HUDSON) == hudson_window
    for r0, rows in RANGES:
        what = f"{key} rows [{r0}, +{rows})"
        assert_route(dev, dm, masks, True, image)
        got = run_two_groups(dev, dm, masks, r0, rows)
        check_two_groups(got, oracle_two_groups(data, None, columns, 1, masks, r0, rows), True, what)
        tiled_opts.setenv("FMH_TILED", "0")
        assert_route(dev, dm, masks, False, image)
        assert window(dev, dm, g2, dev.SWEEP_HUDSON) == hudson_window  # the window is the same on either route
        ref = run_two_groups(dev, dm, masks, r0, rows)
        tiled_opts.setenv("FMH_TILED", "1")
        same_bits(got, ref, what)
        same_totals(got, ref, what)


def one_group(dev, dm, g, r0, rows):
    return dev.population_summaries(dm, g, dev.FORMULA_SPARSE, r0, rows), dev.diversity_sites(dm, g, r0, rows)


def test_one_group_of_every_column(dev, tiled_opts):
    """A single group that holds every column: its counts are the row totals, nothing is counted and no vector is read."""
    columns = 5000
    data, _ = cohort(columns, "5000_a_b", 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    g = dev.Groups(dm, np.ones((1, columns), dtype=np.uint8))
    every = np.arange(columns)
    for r0, rows in RANGES:
        for mode in (dev.SWEEP_SUMMARY, dev.SWEEP_DIVERSITY):
            assert window(dev, dm, g, mode) == (0, 1, 0)
            assert dev.sweep_tiled(dm, g, mode) == (True, image_bytes(S, columns))
        ps, dv = one_group(dev, dm, g, r0, rows)
        sub = data.reshape(S, columns)[r0:r0 + rows].reshape(-1)
        exp = D.region_sweep(sub, None, rows, columns, 1, every, every, D.FORMULA_SPARSE, -1, 16)
        assert np.array_equal(ps.alt[0], exp.alt[0]) and np.array_equal(dv.distinct, exp.distinct[0])
        check_pop(ps.totals[0], exp.pop[0], "summaries")
        check_pop(dv.totals, exp.pop[0], "diversity")
        H.assert_bits_equal(dv.pi, exp.site_pi[0], "pi")
        H.assert_bits_equal(dv.theta, exp.site_theta[0], "theta")
        tiled_opts.setenv("FMH_TILED", "0")
        ps0, dv0 = one_group(dev, dm, g, r0, rows)
        tiled_opts.setenv("FMH_TILED", "1")
        H.assert_bits_equal(dv.pi, dv0.pi, "pi against the row-major route")
        H.assert_bits_equal(dv.theta, dv0.theta, "theta against the row-major route")
        assert np.array_equal(ps.alt, ps0.alt)
        assert {k: bits(v) for k, v in ps.totals[0].items()} == {k: bits(v) for k, v in ps0.totals[0].items()}
        assert {k: bits(v) for k, v in dv.totals.items()} == {k: bits(v) for k, v in dv0.totals.items()}


def oracle_whole_matrix(flat, rows, columns, masks):
    """oracle_two_groups for a matrix of `rows` rows swept whole (that helper's cohorts have S rows)."""
    off = [np.nonzero(m)[0] for m in masks]
    every = np.arange(columns)
    goc = np.where(masks[0] != 0, 0, np.where(masks[1] != 0, 1, 255)).astype(np.uint8)
    return {"sp": D.region_sweep(flat, None, rows, columns, 1, off[0], off[1], D.FORMULA_SPARSE, D.FORMULA_SPARSE, 16),
            "de": D.region_sweep(flat, None, rows, columns, 1, off[0], off[1], D.FORMULA_DENSE, -1, 16),
            "all": D.region_sweep(flat, None, rows, columns, 1, every, every, D.FORMULA_SPARSE, -1, 16),
            "wc": D.wc_sites(flat, None, rows, columns, goc, 2, 1),
            "dense": D.hudson_sweep(flat, None, rows, columns, off[0], off[1], 16)}


@pytest.mark.parametrize("key", ["5000_a_b", "5000_interleaved"])
def test_a_single_partial_tile(dev, tiled_opts, key):
    """37 rows: one image tile, 27 of its rows zero padding, lanes 37 .. 63 clamped to the last row - every sweep of run_two_groups (Hudson dense
    and sparse, summaries, diversity, the fused sweep, the group of every column), one group derived and both counted."""
    rows = 37
    columns, masks, hudson_window = LAYOUTS[key]
    data, _ = D.generate(rows, columns, 77, 0, H.thresholds(rows, 77), masks[1].astype(np.uint8), 0, 16)
    dm = dev.DeviceMatrix.from_host(data, None, rows, columns // 2, 2, 1)
    image = image_bytes(rows, columns)
    assert image == 40 * 1024
    assert window(dev, dm, dev.Groups(dm, masks), dev.SWEEP_HUDSON) == hudson_window
    assert_route(dev, dm, masks, True, image)
    got = run_two_groups(dev, dm, masks, 0, rows)
    check_two_groups(got, oracle_whole_matrix(data, rows, columns, masks), True, f"{key}, 37 rows")
    tiled_opts.setenv("FMH_TILED", "0")
    assert_route(dev, dm, masks, False, image)
    ref = run_two_groups(dev, dm, masks, 0, rows)
    tiled_opts.setenv("FMH_TILED", "1")
    same_bits(got, ref, f"{key}, 37 rows")
    same_totals(got, ref, f"{key}, 37 rows")


def test_default_route_is_the_narrow_window(dev, tiled_opts):
    """FMH_TILED unset: a window of at most seven eighths of the row takes the tiled route (20 and 27 of 40 vectors), a wider one keeps the
    row-major route (39 of 40: two groups that leave the last ten columns out, nothing derived; 40 of 40)."""
    tiled_opts.delenv("FMH_TILED")
    wide = np.stack([span(5000, (0, 2500)), span(5000, (2500, 4990))])
    for key, masks, expect in (("5000_a_b", None, True), ("5000_no_partition", None, True), ("39 of 40", wide, False), ("5000_interleaved", None, False)):
        columns = 5000
        masks = LAYOUTS[key][1] if masks is None else masks
        data, _ = D.generate(64, columns, 5, 0, H.thresholds(64, 5), masks[1].astype(np.uint8), 0, 16)
        dm = dev.DeviceMatrix.from_host(data, None, 64, columns // 2, 2, 1)
        g = dev.Groups(dm, masks)
        if key == "39 of 40":
            assert window(dev, dm, g, dev.SWEEP_HUDSON) == (0, 39, -1)
        assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (expect, image_bytes(64, columns)), key


@pytest.mark.parametrize("key", ["5000_a_b", "5000_interleaved"])
def test_sweeps_under_the_default_route(dev, tiled_opts, key):
    """FMH_TILED unset, every sweep of run_two_groups: windows of at most seven eighths of the row go through the tiled kernels, the
    whole row through the row-major ones; the oracle's results, and the bits of FMH_TILED=0, on either."""
    tiled_opts.delenv("FMH_TILED")
    columns, masks, hudson_window = LAYOUTS[key]
    data, _ = cohort(columns, key, 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    g2 = dev.Groups(dm, masks)
    narrow = hudson_window[1] * 8 <= (columns + 127) // 128 * 7
    assert dev.sweep_tiled(dm, g2, dev.SWEEP_HUDSON) == (narrow, image_bytes(S, columns))
    assert dev.sweep_tiled(dm, g2, dev.SWEEP_REGION) == (narrow, image_bytes(S, columns))
    for r0, rows in RANGES:
        what = f"{key} rows [{r0}, +{rows}), default route"
        got = run_two_groups(dev, dm, masks, r0, rows)
        check_two_groups(got, oracle_two_groups(data, None, columns, 1, masks, r0, rows), True, what)
        tiled_opts.setenv("FMH_TILED", "0")
        ref = run_two_groups(dev, dm, masks, r0, rows)
        tiled_opts.delenv("FMH_TILED")
        same_bits(got, ref, what)
        same_totals(got, ref, what)


@pytest.mark.parametrize("kind", ["missing", "max_allele_2"])
def test_no_image_on_missing_calls_and_on_multi_allelic_rows(dev, tiled_opts, kind):
    """The same cohort with 1 % missing calls, and with alleles up to 2: no image, the row-major routes, the oracle's results."""
    columns, masks, _ = LAYOUTS["5000_a_b"]
    if kind == "missing":
        data, words = cohort(columns, "5000_a_b", 1000 + columns, 0.01)
        declared = 1
    else:
        data, words = cohort(columns, "5000_a_b", 1000 + columns)
        data = data.copy().reshape(S, columns)
        rng = np.random.default_rng(5)
        rows = rng.choice(S, size=S // 20, replace=False)
        data[rows[:, None], rng.integers(0, columns, size=(rows.size, 40))] = 2
        data[0, 0] = 2
        data, declared = data.reshape(-1), 2
    dm = dev.DeviceMatrix.from_host(data, words, S, columns // 2, 2, declared)
    assert_route(dev, dm, masks, False, 0)
    got = run_two_groups(dev, dm, masks, 0, S)
    check_two_groups(got, oracle_two_groups(data, words, columns, declared, masks, 0, S), declared <= 1, kind)


def test_image_follows_every_pack(dev, tiled_opts):
    """Generate, pack, sweep; generate with another seed, pack, sweep: the second sweep is the second cohort's, so a stale image would fail.
    A pack with FMH_TILED_PLANES=0 drops the image; FMH_TILED_BYTES=1 refuses it under the default policy: the same results either way."""
    columns, masks, hudson_window = LAYOUTS["5000_a_b"]
    poc = masks[1].astype(np.uint8)
    off = [np.nonzero(m)[0] for m in masks]
    dm = dev.DeviceMatrix.alloc(S, columns // 2, 2, with_missing=False)
    g = dev.Groups(dm, masks)

    def check(exp, what):
        got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
        assert np.array_equal(got.sites["alt"], exp.alt), what
        for k in TRACKS:
            H.assert_bits_equal(got.sites[k], getattr(exp, k), f"{k} {what}")
        assert H.rel_close(got.totals["numerator_sum"], exp.totals["numerator_sum"]) and H.rel_close(got.totals["denominator_sum"], exp.totals["denominator_sum"])
        return got

    for seed in (11, 12):
        thr = H.thresholds(S, seed)
        dm.generate(seed, 0, thr, poc, 0)
        dm.pack(release_bytes=False)
        assert window(dev, dm, g, dev.SWEEP_HUDSON) == hudson_window
        assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (True, image_bytes(S, columns))
        hdata, _ = D.generate(S, columns, seed, 0, thr, poc, 0, 16)
        exp = D.hudson_sweep(hdata, None, S, columns, off[0], off[1], 16)
        tiled = check(exp, f"seed {seed}")
    tiled_opts.setenv("FMH_TILED_PLANES", "0")
    dm.pack(release_bytes=False)
    tiled_opts.setenv("FMH_TILED_PLANES", "2")  # sweeps would use an image again - but the last pack kept none
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (False, 0)
    plain = check(exp, "no image")
    for k in TRACKS:
        H.assert_bits_equal(plain.sites[k], tiled.sites[k], f"{k} without the image")
    assert {k: bits(v) for k, v in plain.totals.items()} == {k: bits(v) for k, v in tiled.totals.items()}
    tiled_opts.setenv("FMH_TILED_PLANES", "1")  # the default policy (4 517 rows: large enough) with a budget of one byte
    tiled_opts.setenv("FMH_TILED_BYTES", "1")
    dm.pack(release_bytes=False)
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (False, 0)
    refused = check(exp, "image refused")
    assert {k: bits(v) for k, v in refused.totals.items()} == {k: bits(v) for k, v in tiled.totals.items()}
    tiled_opts.delenv("FMH_TILED_BYTES")
    dm.pack(release_bytes=False)
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (True, image_bytes(S, columns))
    check(exp, "image back under the default policy")


def test_pipelined_sharded_sweeps_on_a_local_communicator(dev, tiled_opts):
    """fmh_hudson_sweep_sharded_begin / _end on a local communicator, three steps in flight: the totals of the blocking sweep."""
    from ferromic_amd import _abi, sharding

    lib = _abi.load()
    columns, masks, _ = LAYOUTS["5000_a_b"]
    data, _ = cohort(columns, "5000_a_b", 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    g = dev.Groups(dm, masks)
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON) == (True, image_bytes(S, columns))
    plain = _abi.HudsonTotals()
    _abi.check(lib.fmh_hudson_sweep(dm._h, g._h, 0, S, _abi.FORMULA_DENSE, None, C.byref(plain), None))
    comm = sharding.Comm.local(0)
    for _ in range(3):
        _abi.check(lib.fmh_hudson_sweep_sharded_begin(comm._h, dm._h, g._h, 0, S, _abi.FORMULA_DENSE, None, None))
    for _ in range(3):
        got = _abi.HudsonTotals()
        _abi.check(lib.fmh_hudson_sweep_sharded_end(comm._h, C.byref(got)))
        for k, _t in _abi.HudsonTotals._fields_:
            if k != "pop":
                assert getattr(got, k) == getattr(plain, k), k
        for p in range(2):
            for k, _t in _abi.PopTotals._fields_:
                assert getattr(got.pop[p], k) == getattr(plain.pop[p], k), (p, k)
    comm.close()
