"""The column window of the packed biallelic sweeps: a sweep reads only the 128-column vectors its groups have members in, and when one
or two groups partition the columns of a matrix with nothing missing, one group is not counted at all - its alt count is the row total
(a table of the resident matrix) minus the other group's.

Every case compares with the C oracle (oracle/dense.py) on the same bytes: counts and integer totals exactly, per-site f64 tracks bit for
bit, regional f64 sums to 1e-9; the same sweeps with FMH_COLUMN_WINDOW=0 are a second reference for the per-site bits.  Every case also
asks fmh_sweep_window what the sweep reads and which group it derives, so that a case which silently fell back does not count.

All cases: 64 * 70 + 37 rows, FMH_COLUMN_WINDOW=2 (row totals at any size), FMH_GRID_BLOCKS=1 (each wave walks about 18 tiles: one full
16-deep deferral chunk and a partial one), and a second sweep over rows [13, 13 + 3 000).

These are hand-picked layouts; tests/test_gpu_window_geometry.py covers every window width 1 .. 64, first vectors on both ends and inside, row
ranges around tile edges and other grids with the helpers of this file."""

import ctypes as C
import functools

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.test_gpu_scale_sparse import TRACKS, check_fused_sites, check_fused_totals, check_hud_totals, check_hudson_sites, check_pop, fused

pytestmark = pytest.mark.gpu

S = 64 * 70 + 37
R0, RN = 13, 3000
RANGES = ((0, S), (R0, RN))
DENSE_SUMS = ("numerator_sum", "denominator_sum", "pi1_sum", "pi2_sum", "dxy_sum_all", "site_num_sum", "site_den_sum")


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture
def window_opts(fmh_opts):
    fmh_opts.setenv("FMH_COLUMN_WINDOW", "2")
    fmh_opts.setenv("FMH_GRID_BLOCKS", "1")
    return fmh_opts


def span(columns, *ranges):
    m = np.zeros(columns, dtype=np.uint8)
    for a, b in ranges:
        m[a:b] = 1
    return m


def split(columns, cut, swap=False):
    masks = np.stack([span(columns, (0, cut)), span(columns, (cut, columns))])
    return masks[::-1].copy() if swap else masks


def interleaved(columns):
    even = (np.arange(columns) // 2 % 2 == 0).astype(np.uint8)  # even samples | odd samples
    return np.stack([even, 1 - even])


def hull(masks, skip=None):
    """(first vector, vectors) spanned by the members of the groups other than `skip`; one vector when there is none."""
    cols = np.nonzero(np.delete(masks, skip, axis=0).any(axis=0) if skip is not None else masks.any(axis=0))[0]
    if cols.size == 0:
        return 0, 1
    return int(cols[0] >> 7), int((cols[-1] >> 7) - (cols[0] >> 7) + 1)


def expected_window(masks, derive):
    """The issue's rule, restated: the hull of the groups' supports; when one or two groups partition the columns and the mode may derive,
    the group whose removal leaves the shortest range (ties: the second group), if that is shorter than the hull."""
    first, count = hull(masks)
    best = (first, count, -1)
    partition = bool((masks.sum(axis=0) == 1).all())
    if derive and partition and masks.shape[0] <= 2:
        for d in range(masks.shape[0] - 1, -1, -1):
            f, c = hull(masks, d)
            if c < best[1]:
                best = (f, c, d)
    return best


# columns, masks, what the Hudson / summaries / fused sweeps must report (first vector, vectors, derived group)
LAYOUTS = {
    "5000_a_b": (5000, split(5000, 2500), (0, 20, 1)),                 # boundary inside vector 19; window 20 of 40: sixteen -> four lanes
    "5000_b_a": (5000, split(5000, 2500, swap=True), (0, 20, 0)),      # group 0 starts past vector 0 and is the derived one
    "5000_1000_4000": (5000, split(5000, 1000), (0, 8, 1)),            # the derived group is the larger one
    "5000_4000_1000": (5000, split(5000, 4000), (31, 9, 0)),
    "512_256_256": (512, split(512, 256), (0, 2, 1)),                  # boundary on a vector edge; tiny window
    "130_1_129": (130, split(130, 1), (0, 1, 1)),                      # two vectors; the masked tail of the last vector in the row totals
    "130_129_1": (130, split(130, 129), (1, 1, 0)),
    "4224_2048_2176": (4224, split(4224, 2048), (0, 16, 1)),           # a sixteen-lane matrix (33 vectors) whose window is four-lane
    "12000_6000_6000": (12000, split(12000, 6000), (0, 47, 1)),        # sixteen lanes on both sides; 47 is no multiple of lanes x batch
    "5000_no_partition": (5000, np.stack([span(5000, (300, 900)), span(5000, (3000, 3700))]), (2, 27, -1)),  # hull, nothing derived
    "5000_interleaved": (5000, interleaved(5000), (0, 40, -1)),        # a partition, but nothing to skip: the whole row
}


@functools.lru_cache(maxsize=2)
def cohort(columns, key, seed, missing=0.0):
    """Counter-based biallelic rows (the benchmark's generator) whose frequencies differ between the groups of layout `key`."""
    masks = LAYOUTS[key][1] if key in LAYOUTS else None
    poc = (masks[1] if masks is not None and masks.shape[0] > 1 else np.zeros(columns, np.uint8)).astype(np.uint8)
    data, words = D.generate(S, columns, seed, 0, H.thresholds(S, seed), poc, int(missing * (1 << 24)), 16)
    return data, words


def window(dev, dm, g, mode):
    return dev.sweep_window(dm, g, mode)


def run_two_groups(dev, dm, masks, r0, rows):
    g2 = dev.Groups(dm, masks)
    g1 = [dev.Groups(dm, masks[p:p + 1]) for p in range(2)]
    gall = dev.Groups(dm, np.ones((1, dm.columns), dtype=np.uint8))
    return {"dense": dev.hudson_sweep(dm, g2, dev.FORMULA_DENSE, r0, rows),
            "sparse": dev.hudson_sweep(dm, g2, dev.FORMULA_SPARSE, r0, rows),
            "div": [dev.diversity_sites(dm, g, r0, rows) for g in g1],
            "ps": dev.population_summaries(dm, g2, dev.FORMULA_SPARSE, r0, rows),
            "all": dev.population_summaries(dm, gall, dev.FORMULA_SPARSE, r0, rows),
            "alldiv": dev.diversity_sites(dm, gall, r0, rows),
            "fused": {f: fused(dev, dm, g2, r0, rows, f) for f in (dev.FORMULA_DENSE, dev.FORMULA_SPARSE)},
            "wc": dev.wc_sweep(dm, g2, r0, rows)}


def oracle_two_groups(flat, words, columns, declared, masks, r0, rows):
    sub = flat.reshape(S, columns)[r0:r0 + rows].reshape(-1)
    assert words is None or (r0 == 0 and rows == S)
    off = [np.nonzero(m)[0] for m in masks]
    every = np.arange(columns)
    goc = np.where(masks[0] != 0, 0, np.where(masks[1] != 0, 1, 255)).astype(np.uint8)
    out = {"sp": D.region_sweep(sub, words, rows, columns, declared, off[0], off[1], D.FORMULA_SPARSE, D.FORMULA_SPARSE, 16),
           "de": D.region_sweep(sub, words, rows, columns, declared, off[0], off[1], D.FORMULA_DENSE, -1, 16),
           "all": D.region_sweep(sub, words, rows, columns, declared, every, every, D.FORMULA_SPARSE, -1, 16),
           "wc": D.wc_sites(sub, words, rows, columns, goc, 2, 1)}
    if declared <= 1:
        out["dense"] = D.hudson_sweep(sub, words, rows, columns, off[0], off[1], 16)
    return out


def check_wc(got, exp, what):
    nw = exp.sum_a.size
    for k in range(nw):
        H.assert_bits_equal(got.a[k], exp.a[k], f"W&C a slot {k} {what}")
        H.assert_bits_equal(got.b[k], exp.b[k], f"W&C b slot {k} {what}")
        assert np.array_equal(got.state[k], exp.state[k]), (k, what)
        assert H.rel_close(got.sum_a[k], exp.sum_a[k]) and H.rel_close(got.sum_b[k], exp.sum_b[k]), (k, what)
        assert int(got.informative_sites[k]) == int(exp.informative[k]), (k, what)


def check_two_groups(got, exp, bi, what):
    e = exp["sp"]
    check_hudson_sites(got["sparse"].sites, e, slice(None), bi, f"sparse Hudson {what}")
    check_hud_totals(got["sparse"].totals, e.totals, bi, f"sparse Hudson {what}")
    if "dense" in exp:
        d = exp["dense"]
        assert np.array_equal(got["dense"].sites["alt"], d.alt) and np.array_equal(got["dense"].sites["called"], d.called), what
        for k in TRACKS:
            H.assert_bits_equal(got["dense"].sites[k], getattr(d, k), f"dense Hudson {k} {what}")
        for k in DENSE_SUMS:
            assert H.rel_close(got["dense"].totals[k], d.totals[k]), (k, what)
        for k in ("dxy_uncallable_sites", "sites_with_components"):
            assert got["dense"].totals[k] == d.totals[k], (k, what)
        for p in range(2):
            for k in ("segregating_sites", "uncallable_sites"):
                assert got["dense"].pop[p][k] == d.pop[p][k], (k, p, what)
            assert H.rel_close(got["dense"].pop[p]["pi_sum"], d.pop[p]["pi_sum"]), (p, what)
    for f, fu in got["fused"].items():
        check_fused_sites(fu, e, slice(None), bi, f"fused {f} {what}")
        for p in range(2):
            check_pop(fu["pop"][p], (e if f == D.FORMULA_SPARSE else exp["de"]).pop[p], f"fused {f} pop {p} {what}")
        check_hud_totals(fu["totals"], e.totals, bi, f"fused {f} {what}")
    for p in range(2):
        dv = got["div"][p]
        H.assert_bits_equal(dv.pi, e.site_pi[p], f"diversity pi group {p} {what}")
        H.assert_bits_equal(dv.theta, e.site_theta[p], f"diversity theta group {p} {what}")
        assert np.array_equal(dv.called, e.called[p]) and np.array_equal(dv.distinct, e.distinct[p]), (p, what)
        check_pop(dv.totals, e.pop[p], f"diversity group {p} {what}")
        check_pop(got["ps"].totals[p], e.pop[p], f"summaries group {p} {what}")
    assert np.array_equal(got["ps"].called, e.called), what
    if bi:
        assert np.array_equal(got["ps"].alt, e.alt), what
    a = exp["all"]
    check_pop(got["all"].totals[0], a.pop[0], f"summaries of every column {what}")
    check_pop(got["alldiv"].totals, a.pop[0], f"diversity of every column {what}")
    H.assert_bits_equal(got["alldiv"].pi, a.site_pi[0], f"diversity pi of every column {what}")
    H.assert_bits_equal(got["alldiv"].theta, a.site_theta[0], f"diversity theta of every column {what}")
    assert np.array_equal(got["alldiv"].distinct, a.distinct[0]), what
    if bi:
        assert np.array_equal(got["all"].alt[0], a.alt[0]), what
    check_wc(got["wc"], exp["wc"], what)


def same_bits(a, b, what):
    """Two runs of run_two_groups: every per-site array the same bits."""
    for key in ("dense", "sparse"):
        for k in TRACKS:
            H.assert_bits_equal(a[key].sites[k], b[key].sites[k], f"{key} {k} {what}")
        assert np.array_equal(a[key].sites["alt"], b[key].sites["alt"]), (key, what)
    for f in a["fused"]:
        for k in TRACKS:
            H.assert_bits_equal(a["fused"][f]["sites"][k], b["fused"][f]["sites"][k], f"fused {f} {k} {what}")
        for k in ("pi", "theta"):
            for p in range(2):
                H.assert_bits_equal(a["fused"][f][k][p], b["fused"][f][k][p], f"fused {f} {k} {p} {what}")
    for p in range(2):
        H.assert_bits_equal(a["div"][p].pi, b["div"][p].pi, f"diversity pi {p} {what}")
        H.assert_bits_equal(a["div"][p].theta, b["div"][p].theta, f"diversity theta {p} {what}")
    H.assert_bits_equal(a["alldiv"].pi, b["alldiv"].pi, f"diversity pi of every column {what}")
    assert np.array_equal(a["ps"].alt, b["ps"].alt) and np.array_equal(a["all"].alt, b["all"].alt), what
    for k in range(a["wc"].a.shape[0]):
        H.assert_bits_equal(a["wc"].a[k], b["wc"].a[k], f"W&C a {k} {what}")
        H.assert_bits_equal(a["wc"].b[k], b["wc"].b[k], f"W&C b {k} {what}")


def check_windows(dev, dm, masks, hudson_window, active=True):
    """fmh_sweep_window for every sweep run_two_groups makes."""
    whole = (0, (dm.columns + 127) // 128, -1)
    g2 = dev.Groups(dm, masks)
    for mode in (dev.SWEEP_HUDSON, dev.SWEEP_SUMMARY, dev.SWEEP_REGION):
        assert window(dev, dm, g2, mode) == (hudson_window if active else whole), mode
        assert window(dev, dm, g2, mode) == (expected_window(masks, True) if active else whole), mode
    assert window(dev, dm, g2, dev.SWEEP_WC) == ((*hull(masks), -1) if active else whole)  # W&C: the window only
    for p in range(2):
        g1 = dev.Groups(dm, masks[p:p + 1])
        assert window(dev, dm, g1, dev.SWEEP_DIVERSITY) == (expected_window(masks[p:p + 1], True) if active else whole), p
    gall = dev.Groups(dm, np.ones((1, dm.columns), dtype=np.uint8))
    for mode in (dev.SWEEP_SUMMARY, dev.SWEEP_DIVERSITY):  # one group of every column: its counts ARE the row totals; one vector is still read
        assert window(dev, dm, gall, mode) == ((0, 1, 0) if active else whole), mode


@pytest.mark.parametrize("key", list(LAYOUTS))
def test_two_group_layouts(dev, window_opts, key):
    columns, masks, hudson_window = LAYOUTS[key]
    data, _ = cohort(columns, key, 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    check_windows(dev, dm, masks, hudson_window)
    for r0, rows in RANGES:
        what = f"{key} rows [{r0}, +{rows})"
        got = run_two_groups(dev, dm, masks, r0, rows)
        check_two_groups(got, oracle_two_groups(data, None, columns, 1, masks, r0, rows), True, what)
        window_opts.setenv("FMH_COLUMN_WINDOW", "0")
        check_windows(dev, dm, masks, hudson_window, active=False)
        same_bits(got, run_two_groups(dev, dm, masks, r0, rows), what)
        window_opts.setenv("FMH_COLUMN_WINDOW", "2")


def test_four_contiguous_wc_groups_read_their_hull(dev, window_opts):
    """W&C and the summaries of four contiguous groups take the window (the hull of the groups), never a derived group."""
    columns = 5000
    masks = np.stack([span(columns, (600 + 600 * k, 1200 + 600 * k)) for k in range(4)])  # columns [600, 3000): vectors 4 .. 23
    goc = np.full(columns, 255, dtype=np.uint8)
    for k in range(4):
        goc[masks[k] != 0] = k
    data, _ = cohort(columns, "5000_a_b", 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    g = dev.Groups(dm, masks)
    assert window(dev, dm, g, dev.SWEEP_WC) == (4, 20, -1) and window(dev, dm, g, dev.SWEEP_SUMMARY) == (4, 20, -1)
    for r0, rows in RANGES:
        sub = data.reshape(S, columns)[r0:r0 + rows].reshape(-1)
        exp = D.wc_sites(sub, None, rows, columns, goc, 4, 1)
        got = dev.wc_sweep(dm, g, r0, rows)
        check_wc(got, exp, f"rows [{r0}, +{rows})")
        ps = dev.population_summaries(dm, g, dev.FORMULA_SPARSE, r0, rows)
        assert np.array_equal(ps.alt, np.stack([sub.reshape(rows, columns)[:, masks[k] != 0].sum(axis=1, dtype=np.uint32) for k in range(4)]))
        window_opts.setenv("FMH_COLUMN_WINDOW", "0")
        assert window(dev, dm, g, dev.SWEEP_WC) == (0, 40, -1)
        off = dev.wc_sweep(dm, g, r0, rows)
        for k in range(got.a.shape[0]):
            H.assert_bits_equal(got.a[k], off.a[k], f"W&C a {k}")
            H.assert_bits_equal(got.b[k], off.b[k], f"W&C b {k}")
        window_opts.setenv("FMH_COLUMN_WINDOW", "2")


@pytest.mark.parametrize("kind", ["missing", "max_allele_3"])
def test_inactive_on_missing_calls_and_on_multi_allelic_rows(dev, window_opts, kind):
    """The same cohort with 1 % missing calls, and with alleles up to 3: the whole row, nothing derived, the oracle's results."""
    columns, masks, hudson_window = LAYOUTS["5000_a_b"]
    if kind == "missing":
        data, words = cohort(columns, "5000_a_b", 1000 + columns, 0.01)
        declared = 1
    else:
        data, words = cohort(columns, "5000_a_b", 1000 + columns)
        data = data.copy().reshape(S, columns)
        rng = np.random.default_rng(5)
        rows = rng.choice(S, size=S // 20, replace=False)
        data[rows[:, None], rng.integers(0, columns, size=(rows.size, 40))] = rng.integers(2, 4, size=(rows.size, 40), dtype=np.uint8)
        data[0, 0] = 3
        data, declared = data.reshape(-1), 3
    dm = dev.DeviceMatrix.from_host(data, words, S, columns // 2, 2, declared)
    check_windows(dev, dm, masks, hudson_window, active=False)
    got = run_two_groups(dev, dm, masks, 0, S)
    check_two_groups(got, oracle_two_groups(data, words, columns, declared, masks, 0, S), declared <= 1, kind)


def test_row_totals_follow_every_pack(dev, window_opts):
    """Generate, pack, sweep; generate with another seed, pack, sweep: the second sweep is the second cohort's.  A pack with
    FMH_COLUMN_WINDOW=0 after a pack with 2 drops the table: nothing is derived any more."""
    columns, masks, hudson_window = LAYOUTS["5000_a_b"]
    poc = masks[1].astype(np.uint8)
    off = [np.nonzero(m)[0] for m in masks]
    dm = dev.DeviceMatrix.alloc(S, columns // 2, 2, with_missing=False)
    g = dev.Groups(dm, masks)
    for seed in (11, 12):
        thr = H.thresholds(S, seed)
        dm.generate(seed, 0, thr, poc, 0)
        dm.pack(release_bytes=False)
        assert window(dev, dm, g, dev.SWEEP_HUDSON) == hudson_window
        got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
        hdata, _ = D.generate(S, columns, seed, 0, thr, poc, 0, 16)
        exp = D.hudson_sweep(hdata, None, S, columns, off[0], off[1], 16)
        assert np.array_equal(got.sites["alt"], exp.alt), seed
        for k in TRACKS:
            H.assert_bits_equal(got.sites[k], getattr(exp, k), f"{k} seed {seed}")
        assert H.rel_close(got.totals["numerator_sum"], exp.totals["numerator_sum"]) and H.rel_close(got.totals["denominator_sum"], exp.totals["denominator_sum"])
    window_opts.setenv("FMH_COLUMN_WINDOW", "0")
    dm.pack(release_bytes=False)
    window_opts.setenv("FMH_COLUMN_WINDOW", "2")  # sweeps would use a table again - but the last pack kept none
    assert window(dev, dm, g, dev.SWEEP_HUDSON) == (0, 40, -1)
    got = dev.hudson_sweep(dm, g, dev.FORMULA_DENSE)
    assert np.array_equal(got.sites["alt"], exp.alt)


@pytest.mark.parametrize("graph", [False, True])
def test_pipelined_sharded_sweeps_on_a_local_communicator(dev, window_opts, graph):
    """fmh_hudson_sweep_sharded_begin / _end on a local communicator, three steps in flight; the same replayed from a captured graph on an
    explicit stream (FMH_GRAPH=1): the totals of the blocking sweep."""
    from ferromic_amd import _abi, sharding

    lib = _abi.load()
    columns, masks, hudson_window = LAYOUTS["5000_a_b"]
    data, _ = cohort(columns, "5000_a_b", 1000 + columns)
    dm = dev.DeviceMatrix.from_host(data, None, S, columns // 2, 2, 1)
    g = dev.Groups(dm, masks)
    assert window(dev, dm, g, dev.SWEEP_HUDSON) == hudson_window
    plain = _abi.HudsonTotals()
    _abi.check(lib.fmh_hudson_sweep(dm._h, g._h, 0, S, _abi.FORMULA_DENSE, None, C.byref(plain), None))
    comm = sharding.Comm.local(0)
    stream = None
    if graph:
        window_opts.setenv("FMH_GRAPH", "1")
        # a non-blocking stream of the caller's own (the NULL stream cannot be captured), from the HIP runtime the library has loaded
        hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        stream = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    ptr = stream
    for _ in range(2):  # the second round replays what the first one captured
        for _ in range(3):
            _abi.check(lib.fmh_hudson_sweep_sharded_begin(comm._h, dm._h, g._h, 0, S, _abi.FORMULA_DENSE, None, ptr))
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
    if stream is not None:
        assert hip.hipStreamDestroy(stream) == 0
