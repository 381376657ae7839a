"""The per-site epilogue of the table form of the tiled sweep (site_const_epilogue.hpp): every called count of that
form is a launch constant, so its divisions share refined reciprocals computed once per workgroup, its integer sums are 32 bits wide and
its formula pair is resolved by the launcher.  It must give the bits of finish_biallelic_site + site_epilogue.

Everything is bit for bit; there is no tolerance anywhere in this file.  Two references:
  * the same process with FMH_PREFIX_COUNTS=0 (the window of the tiled route, the old epilogue) at an equal grid (FMH_GRID_BLOCKS): every
    per-site track and every field of the totals;
  * the C oracle (oracle/dense.py) on the same bytes: every per-site value (check_two_groups; the oracle's regional sums have another
    order of additions and stay with that helper's contract).
Every case asks fmh_sweep_prefix whether the sweeps really take the table form (and that they do not under FMH_PREFIX_COUNTS=0).

Modes and instantiations: run_two_groups makes the Hudson sweep with the dense and the sparse formula (mode 3), the summaries of two
groups and of one (mode 1), the diversity of one group (mode 5) and the fused region sweep with the dense and the sparse summary formula
under the sparse Hudson set (mode 7: a distinct pair and an equal one); more_sweeps adds the third formula for each of them and the fused
sweep without a Hudson part (mode 5 with two groups)."""

import ctypes as C
import struct

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.test_gpu_column_window import check_two_groups, run_two_groups, same_bits, span
from tests.test_gpu_prefix_counts import assert_routes, table_bytes
from tests.test_gpu_scale_sparse import TRACKS, unpack_fused
from tests.test_gpu_tiled_planes import oracle_whole_matrix, same_totals

pytestmark = pytest.mark.gpu

SITE_FIELDS = TRACKS + ("alt", "called")


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture
def opts(fmh_opts):
    fmh_opts.setenv("FMH_TILED_PLANES", "2")
    fmh_opts.setenv("FMH_PREFIX_COUNTS", "2")
    fmh_opts.setenv("FMH_COLUMN_WINDOW", "2")
    fmh_opts.setenv("FMH_TILED", "1")
    fmh_opts.setenv("FMH_GRID_BLOCKS", "1")
    return fmh_opts


def bits(v):
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, np.ndarray):
        return v.tobytes()
    return v


def hudson_with(dev, dm, g, formula, r0, rows, keep=SITE_FIELDS):
    """fmh_hudson_sweep with only the tracks of `keep` requested (the other pointers NULL): the tracks and every total, as bytes."""
    from ferromic_amd import _abi

    bufs = {k: dev.DeviceBuffer(dm.device, 8 * rows) for k in SITE_FIELDS if k in keep}
    sites = _abi.HudsonSites(*(bufs[k].ptr if k in bufs else None for k in SITE_FIELDS))
    tot = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_hudson_sweep(dm._h, g._h, r0, rows, formula, C.byref(sites), C.byref(tot), None))
    out = {k: bufs[k].to_numpy(np.uint64, rows).tobytes() for k in bufs}
    out["totals"] = {k: bits(v) for k, v in dev.hudson_totals_dict(tot).items()}
    out["pop"] = [{k: bits(getattr(tot.pop[p], k)) for k, _t in _abi.PopTotals._fields_} for p in range(2)]
    return out


def region(dev, dm, g2, r0, rows, summary_formula, hudson_formula):
    """fmh_pair_region_sweep with any formula pair (hudson_formula -1: no Hudson part, the two-group diversity sweep)."""
    from ferromic_amd import _abi

    bufs = {k: dev.DeviceBuffer(dm.device, 16 * rows) for k in ("pi", "theta")}
    bufs.update({k: dev.DeviceBuffer(dm.device, 8 * rows) for k in SITE_FIELDS})
    div = _abi.PairDiversitySites(bufs["pi"].ptr, bufs["theta"].ptr)
    sites = _abi.HudsonSites(*(bufs[k].ptr for k in SITE_FIELDS))
    tot = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_pair_region_sweep(dm._h, g2._h, r0, rows, summary_formula, hudson_formula, C.byref(div), C.byref(sites),
                                                 C.byref(tot), None))
    fu = unpack_fused(dev, bufs, tot, rows)
    out = {k: fu[k].tobytes() for k in ("pi", "theta")}
    out.update({k: fu["sites"][k].tobytes() for k in (SITE_FIELDS if hudson_formula >= 0 else ("alt", "called"))})
    out["totals"] = {k: bits(v) for k, v in fu["totals"].items()} if hudson_formula >= 0 else None
    out["pop"] = [{k: bits(v) for k, v in fu["pop"][p].items()} for p in range(2)]
    return out


def more_sweeps(dev, dm, masks, r0, rows):
    """What run_two_groups leaves out: the third formula on every entry point, every formula for the summaries, the fused sweep's other
    distinct pairs and the fused sweep without a Hudson part.  Everything as bytes: two runs compare with ==."""
    g2 = dev.Groups(dm, masks)
    out = {"hudson summary formula": hudson_with(dev, dm, g2, dev.FORMULA_SUMMARY, r0, rows)}
    for f in (dev.FORMULA_DENSE, dev.FORMULA_SUMMARY):
        ps = dev.population_summaries(dm, g2, f, r0, rows)
        out["summaries", f] = ([{k: bits(v) for k, v in t.items()} for t in ps.totals], ps.alt.tobytes(), ps.called.tobytes())
        ps1 = dev.population_summaries(dm, dev.Groups(dm, masks[:1]), f, r0, rows)
        out["summaries of group 0", f] = ([{k: bits(v) for k, v in t.items()} for t in ps1.totals], ps1.alt.tobytes())
    for sf, hf in ((dev.FORMULA_SUMMARY, dev.FORMULA_SUMMARY), (dev.FORMULA_SUMMARY, dev.FORMULA_SPARSE), (dev.FORMULA_SPARSE, dev.FORMULA_DENSE),
                   (dev.FORMULA_DENSE, dev.FORMULA_DENSE), (dev.FORMULA_DENSE, -1), (dev.FORMULA_SPARSE, -1), (dev.FORMULA_SUMMARY, -1)):
        out["region", sf, hf] = region(dev, dm, g2, r0, rows, sf, hf)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k] == b[k], (k, what)


def both_epilogues(dev, opts, dm, masks, r0, rows, what):
    """The sweeps on the table form and, at the same grid, under FMH_PREFIX_COUNTS=0: the same bits everywhere.  Returns the table form's."""
    table = table_bytes(dm.variants, dm.columns)
    g2 = dev.Groups(dm, masks)
    assert assert_routes(dev, dm, masks, table), what
    for mode in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION):
        assert dev.sweep_prefix(dm, g2, mode)[0] is True, (mode, what)
    got, more = run_two_groups(dev, dm, masks, r0, rows), more_sweeps(dev, dm, masks, r0, rows)
    opts.setenv("FMH_PREFIX_COUNTS", "0")  # read at every sweep: the window of the tiled route and the old epilogue, the table still present
    assert_routes(dev, dm, masks, table, on=False)
    ref, more_ref = run_two_groups(dev, dm, masks, r0, rows), more_sweeps(dev, dm, masks, r0, rows)
    opts.setenv("FMH_PREFIX_COUNTS", "2")
    same_bits(got, ref, what)
    same_totals(got, ref, what)
    assert_same(more, more_ref, what)
    return got


# ---- every numerator of every shared division, for one n at a time -------------------------------------------------------------------------
SIZES = ((2, 2), (2, 3), (3, 7), (127, 129), (1000, 1001), (2500, 2500), (4093, 2))


def ramp_matrix(n1, n2, layout, swapped, seed):
    """n1 + 1 rows: row i has i alternate calls among the n1 columns of population 1 (every numerator a / n1, a r / (n1 (n1 - 1)), ssq / n1^2
    and a1 r2 + r1 a2 of that size); population 2's count is random and takes 0 and n2.  `swapped`: population 1 is the second group.
    Layouts: 'derived' - the groups partition the row, one comes from the row totals; 'inside' - both counted, ranges that start and end
    inside vectors; 'boundary' - both counted, both ranges start on a vector boundary."""
    na, nb = (n2, n1) if swapped else (n1, n2)
    if layout == "derived":
        ra, rb = (0, na), (na, na + nb)
        columns = na + nb
    elif layout == "inside":
        ra, rb = (3, 3 + na), (5 + na, 5 + na + nb)
        columns = 6 + na + nb
    else:
        start = (na + 128) // 128 * 128  # the first boundary past group a's last column
        ra, rb = (0, na), (start, start + nb)
        columns = start + nb
    rows = n1 + 1
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, size=(rows, columns), dtype=np.uint8)
    r1, r2 = (rb, ra) if swapped else (ra, rb)
    c2 = rng.integers(0, n2 + 1, size=rows)
    c2[0], c2[-1] = n2, 0
    if rows > 2:
        c2[1] = 0
        c2[rows // 2] = n2
    for i in range(rows):
        data[i, r1[0]:r1[1]] = rng.permutation(np.arange(n1) < i)
        data[i, r2[0]:r2[1]] = rng.permutation(np.arange(n2) < c2[i])
    return columns, np.stack([span(columns, ra), span(columns, rb)]), data


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("layout", ["derived", "inside", "boundary"])
@pytest.mark.parametrize("sizes", SIZES)
def test_every_numerator_of_one_group_size(dev, opts, sizes, layout, swapped):
    n1, n2 = sizes
    columns, masks, data = ramp_matrix(n1, n2, layout, swapped, 1000 * n1 + n2)
    rows = n1 + 1
    what = f"n = {sizes}, {layout}, swapped {swapped}"
    assert sorted(int(m.sum()) for m in masks) == sorted(sizes)
    dm = dev.DeviceMatrix.from_host(data.reshape(-1), None, rows, columns, 1, 1)
    derived = dev.sweep_window(dm, dev.Groups(dm, masks), dev.SWEEP_HUDSON)[2]
    # (a partition inside one vector derives nothing: no group's removal shortens the window - both are then counted from the table)
    assert (derived >= 0) == (layout == "derived" and columns > 128), what
    got = both_epilogues(dev, opts, dm, masks, 0, rows, what)
    alt1 = got["dense"].sites["alt"][1 if swapped else 0]
    assert np.array_equal(alt1, np.arange(rows)), what  # every numerator was there
    check_two_groups(got, oracle_whole_matrix(data.reshape(-1), rows, columns, masks), True, what)


# ---- the 32-bit edge --------------------------------------------------------------------------------------------------------------------------
def edge_rows(rows, columns, seed):
    data = np.random.default_rng(seed).integers(0, 2, size=(rows, columns), dtype=np.uint8)
    data[0] = 0
    data[1] = 1
    data[2] = 0
    data[2, 40000] = 1        # one alternate call, in the second group
    data[3] = 0
    data[3, 5] = 1            # one, in the first
    data[4] = 1
    data[4, 77] = 0           # n - 1 of the first group, all of the second
    data[5] = 1
    data[5, columns - 1] = 0  # all of the first, n - 1 of the second
    data[64] = 1              # the extremes again in the second tile and in the partial third one
    data[129] = 0
    return data


def test_largest_32_bit_products(dev, opts):
    """65 535 columns, the widest row that has a table: groups of 32 768 and 32 767 (n1 n2, n (n - 1) and the sums of squares next to 2^30) for
    the Hudson and the fused sweeps, and ONE group of all 65 535 columns counted from the table (FMH_COLUMN_WINDOW=0 at the sweep: nothing is
    derived) for the summaries and the diversity sweep: an all-alt or all-ref row has ssq = 65 535^2, the largest u32 the route can meet."""
    rows, columns = 130, 65535
    data = edge_rows(rows, columns, 65535)
    masks = np.stack([span(columns, (0, 32768)), span(columns, (32768, columns))])
    dm = dev.DeviceMatrix.from_host(data.reshape(-1), None, rows, columns, 1, 1)
    for m in (masks, masks[::-1].copy()):
        got = both_epilogues(dev, opts, dm, m, 0, rows, "65 535 columns")
        check_two_groups(got, oracle_whole_matrix(data.reshape(-1), rows, columns, m), True, "65 535 columns")
    every = np.arange(columns)
    exp = D.region_sweep(data.reshape(-1), None, rows, columns, 1, every, every, D.FORMULA_SPARSE, -1, 16)
    gall = dev.Groups(dm, np.ones((1, columns), dtype=np.uint8))
    opts.setenv("FMH_COLUMN_WINDOW", "0")  # no derived group: the one group is counted - boundary pvec of the table
    runs = {}
    for side in ("2", "0"):
        opts.setenv("FMH_PREFIX_COUNTS", side)
        for mode in (dev.SWEEP_SUMMARY, dev.SWEEP_DIVERSITY):
            assert dev.sweep_prefix(dm, gall, mode)[0] is (side == "2"), (mode, side)
        dv = dev.diversity_sites(dm, gall, 0, rows)
        ps = {f: dev.population_summaries(dm, gall, f, 0, rows) for f in (dev.FORMULA_SPARSE, dev.FORMULA_DENSE, dev.FORMULA_SUMMARY)}
        runs[side] = {"pi": dv.pi.tobytes(), "theta": dv.theta.tobytes(), "distinct": dv.distinct.tobytes(), "called": dv.called.tobytes(),
                      "div totals": {k: bits(v) for k, v in dv.totals.items()},
                      "summaries": {f: ([{k: bits(v) for k, v in t.items()} for t in p.totals], p.alt.tobytes()) for f, p in ps.items()}}
        H.assert_bits_equal(dv.pi, exp.site_pi[0], f"pi of all 65 535 columns, table {side}")
        H.assert_bits_equal(dv.theta, exp.site_theta[0], f"theta of all 65 535 columns, table {side}")
        assert np.array_equal(ps[dev.FORMULA_SPARSE].alt[0], exp.alt[0]) and ps[dev.FORMULA_SPARSE].alt[0][1] == 65535
    opts.setenv("FMH_PREFIX_COUNTS", "2")
    opts.setenv("FMH_COLUMN_WINDOW", "2")
    assert_same(runs["2"], runs["0"], "one group of 65 535 columns")


def test_65536_columns_keep_the_old_epilogue(dev, opts):
    """One column more: no table (u16 entries), so no table form and none of the 32-bit arithmetic; the sweep is the window's, the oracle's bits."""
    rows, columns = 65, 65536
    data = edge_rows(130, columns, 65536)[:rows]
    masks = np.stack([span(columns, (0, 32768)), span(columns, (32768, columns))])
    dm = dev.DeviceMatrix.from_host(data.reshape(-1), None, rows, columns, 1, 1)
    g = dev.Groups(dm, masks)
    for mode in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION):
        assert dev.sweep_prefix(dm, g, mode)[0] is False and dev.sweep_prefix(dm, g, mode)[2] == 0
    assert dev.sweep_tiled(dm, g, dev.SWEEP_HUDSON)[0] is True
    got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
    off = [np.nonzero(m)[0] for m in masks]
    exp = D.hudson_sweep(data.reshape(-1), None, rows, columns, off[0], off[1], 16)
    assert np.array_equal(got.sites["alt"], exp.alt)
    for k in TRACKS:
        H.assert_bits_equal(got.sites[k], getattr(exp, k), f"{k} at 65 536 columns")


# ---- degenerate sizes, tile shapes, grids, row ranges ---------------------------------------------------------------------------------------
SHAPES = {"one column | rest": [(0, 1), (1, 250)],                # derived: pi NaN tracks, pop_unc, no components
          "rest | one column": [(0, 249), (249, 250)],
          "one column and a range, both counted": [(130, 131), (3, 90)],
          "two single columns": [(7, 8), (200, 201)],
          "halves": [(0, 125), (125, 250)],
          "two inner ranges": [(20, 140), (150, 249)]}


@pytest.mark.parametrize("rows", (63, 64, 65, 130))
def test_tile_shapes_grids_and_degenerate_groups(dev, opts, rows):
    """63, 64, 65 and 130 rows; grids of 1 and 3 workgroups; the whole matrix and a row range that starts inside an image tile (every 64-row
    tile of the sweep then straddles two image tiles); a group of ONE column (n == 1: pi is NaN on the tracks, every site uncallable for the
    population, no Hudson components) on either side, derived and counted."""
    columns = 250
    r0 = 13 if rows > 65 else 5
    for name, ranges in SHAPES.items():
        masks = np.stack([span(columns, r) for r in ranges])
        data, _ = D.generate(rows, columns, 300 + rows, 0, H.thresholds(rows, 7), masks[1].astype(np.uint8), 0, 16)
        dm = dev.DeviceMatrix.from_host(data, None, rows, columns, 1, 1)
        for a, n in ((0, rows), (r0, rows - r0 - 2)):
            exp = oracle_whole_matrix(data.reshape(rows, columns)[a:a + n].reshape(-1), n, columns, masks)
            for grid in ("1", "3"):
                what = f"{rows} rows, {name}, rows [{a}, +{n}), grid {grid}"
                opts.setenv("FMH_GRID_BLOCKS", grid)
                got = both_epilogues(dev, opts, dm, masks, a, n, what)
                check_two_groups(got, exp, True, what)
                if "one column" in name or "single" in name:
                    p = [int(m.sum()) for m in masks].index(1)
                    assert np.isnan(got["dense"].sites["pi2" if p else "pi1"]).all() and np.isnan(got["dense"].sites["num"]).all(), what
                    assert got["dense"].pop[p]["uncallable_sites"] == n and got["dense"].totals["sites_with_components"] == 0, what
                    assert np.isnan(got["div"][p].pi).all() and np.isnan(got["div"][p].theta).all(), what


def test_an_empty_group_never_takes_the_table_form(dev, opts):
    """fmh_groups_create accepts a group without members, but such a group is no column range and is never the derived one (removing it
    does not shorten the window), so it is always counted and the plan keeps the window: the new epilogue never sees n == 0."""
    rows, columns = 65, 250
    data, _ = D.generate(rows, columns, 5, 0, H.thresholds(rows, 5), np.zeros(columns, np.uint8), 0, 16)
    dm = dev.DeviceMatrix.from_host(data, None, rows, columns, 1, 1)
    empty, every, part = np.zeros(columns, np.uint8), np.ones(columns, np.uint8), span(columns, (0, 100))
    for masks in ([empty, every], [every, empty], [empty, part], [part, empty]):
        g = dev.Groups(dm, np.stack(masks))
        for mode in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION):
            assert dev.sweep_prefix(dm, g, mode)[0] is False, mode
    for mode in (dev.SWEEP_SUMMARY, dev.SWEEP_DIVERSITY):
        assert dev.sweep_prefix(dm, dev.Groups(dm, empty[None]), mode)[0] is False, mode


# ---- null tracks --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formula", ["dense", "sparse"])
def test_null_tracks_change_nothing_else(dev, opts, formula):
    """fst = num / dxy is computed only when its track is requested: with fst NULL, and with each other track pointer NULL in turn, the
    remaining tracks and every total keep their bits - and the full set is the old epilogue's."""
    rows, columns = 130, 250
    f = dev.FORMULA_DENSE if formula == "dense" else dev.FORMULA_SPARSE
    for ranges in ([(0, 125), (125, 250)], [(20, 140), (150, 249)]):
        masks = np.stack([span(columns, r) for r in ranges])
        data, _ = D.generate(rows, columns, 41, 0, H.thresholds(rows, 41), masks[1].astype(np.uint8), 0, 16)
        dm = dev.DeviceMatrix.from_host(data, None, rows, columns, 1, 1)
        g = dev.Groups(dm, masks)
        for r0, n in ((0, rows), (13, 100)):
            assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON)[0] is True
            full = hudson_with(dev, dm, g, f, r0, n)
            assert np.isfinite(np.frombuffer(full["fst"], dtype=np.float64)).any()
            opts.setenv("FMH_PREFIX_COUNTS", "0")
            assert dev.sweep_prefix(dm, g, dev.SWEEP_HUDSON)[0] is False
            assert_same(full, hudson_with(dev, dm, g, f, r0, n), f"{formula} every track, old epilogue")
            opts.setenv("FMH_PREFIX_COUNTS", "2")
            for gone in SITE_FIELDS:
                part = hudson_with(dev, dm, g, f, r0, n, keep=tuple(k for k in SITE_FIELDS if k != gone))
                assert gone not in part
                assert_same(part, {k: v for k, v in full.items() if k != gone}, f"{formula} without {gone}, rows [{r0}, +{n})")
            none = hudson_with(dev, dm, g, f, r0, n, keep=())
            assert_same(none, {k: full[k] for k in ("totals", "pop")}, f"{formula} without any track")
