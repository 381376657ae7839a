"""LD clumping on the device (fmh_clump, fmh_geno_ld_pairs) against tests/clump_ref.py, the oracle written from the definition, and against
the host twin (fmh_clump_host): the assignment and the clump count with array_equal, r^2 bit for bit (NaN included), the pair counts as
integers.  Cohorts are founder mosaics (neighbouring sites in LD) uploaded as bit planes with RANDOM bits under the uncalled entries
(tests/test_gpu_sfs.py's upload): the kernels have to mask them with the called plane.  The outputs are pre-filled with junk by
ferromic_amd.device.clump: every entry has to be WRITTEN.

Shapes are the smallest at which the kernels can go wrong: selected sample counts around the 16 samples of a word and the 64 of a 16-byte
fragment, over one and several K slabs (a slab is 256 samples), sample lists that start late or skip; participant counts around one and two
64-participant tiles and about 300 (five tiles, candidate tiles of 32 and 64); no, one, every third and every site a candidate; windows of
nothing, a few sites and everything; both cores and every matrix kind; chunks, grids and a caller's stream."""

import ctypes as C

import numpy as np
import pytest

from tests import clump_ref as R
from tests.ibd_ref import genotypes_from_dosages
from tests.test_gpu_sfs import KINDS, upload

pytestmark = pytest.mark.gpu

BASE = R.params(p1=0.03, p2=0.1, r2=0.3, window=90)   # about 60 sites wide: positions step by 1.5 on average
ROWS, SAMPLES = 300, 200


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


_cohorts, _oracle = {}, {}


def cohort(kind, seed=1, rows=ROWS, samples=SAMPLES):
    """(alleles, called or None, dosages [rows][samples], positions, p) of a mosaic cohort as a matrix kind can hold it, made once."""
    key = (kind, seed, rows, samples)
    if key not in _cohorts:
        max_allele, missing = KINDS[kind]
        d = R.mosaic_dosages(rows, samples, seed, miss=0.04 if (missing or max_allele > 1) else 0.0)
        x, called = genotypes_from_dosages(d, seed, high_allele=max_allele, uncalled=missing)
        pos, p = R.mosaic_positions(rows, seed), R.mosaic_p(rows, seed)
        for a in (x, called, d, pos, p):
            a.setflags(write=False)
        _cohorts[key] = (x, called if missing else None, d, pos, p)
    return _cohorts[key]


def matrix(dev, kind, seed=1, planes=True, rows=ROWS, samples=SAMPLES):
    x, called, d, pos, p = cohort(kind, seed, rows, samples)
    return upload(dev, x, called, KINDS[kind][0], planes=planes, ploidy=2)


def oracle(key, dosage, x, p, prm):
    """The oracle's answer, computed once per request and shared."""
    key = (key, tuple(sorted(prm.items())))
    if key not in _oracle:
        _oracle[key] = R.clump(dosage, x, p, prm)
    return _oracle[key]


def clump_and_check(dev, dm, kind, prm, what, seed=1, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, p=None, pos="own", twin=True,
                    stream=None, rows=ROWS):
    """fmh_clump against the oracle (and the twin) over the same kept rows and samples; returns the oracle's result."""
    _, _, d, own_pos, own_p = cohort(kind, seed, rows)
    pos = own_pos if isinstance(pos, str) else pos
    p = own_p if p is None else p
    count = d.shape[0] - row_begin if row_count is None else row_count
    rel = np.arange(count) if keep is None else np.flatnonzero(np.asarray(keep, dtype=bool))
    cols = np.arange(d.shape[1] if n_samples is None else n_samples) if samples is None else np.asarray(samples)
    dosage = np.ascontiguousarray(d[row_begin + rel][:, cols])
    x = None if pos is None else pos[row_begin + rel] - (pos[row_begin] if count else 0)
    p_range = np.ascontiguousarray(p[row_begin:row_begin + count])
    key = (kind, seed, rows, row_begin, count, None if keep is None else rel.tobytes(), cols.tobytes(), pos is None or pos.tobytes(), p_range.tobytes())
    ref = oracle(key, dosage, x, p_range[rel], prm)
    want_index, want_r2 = np.full(count, -1, dtype=np.int64), np.full(count, np.nan)
    owned = ref["index_of"] >= 0
    want_index[rel[owned]] = rel[ref["index_of"][owned]]
    want_r2[rel] = ref["r2"]
    positions = None
    if pos is not None:
        positions = np.zeros(dm.variants, dtype=np.uint32)
        positions[row_begin:row_begin + count] = pos[row_begin:row_begin + count] - (pos[row_begin] if count else 0)
    got = dev.clump(dm, p_range, dev.clump_params(**prm), samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=row_count, keep=keep,
                    positions=positions, stream=stream)
    index = np.where(got.index_of == dev.CLUMP_NONE, -1, got.index_of.astype(np.int64))
    assert np.array_equal(index, want_index), (what, np.flatnonzero(index != want_index)[:8])
    assert R.same_bits(got.r2, want_r2), what
    assert got.n_clumps == ref["n_clumps"], what
    if twin:
        host = dev.clump_host(dosage, p_range[rel], dev.clump_params(**prm), x=x)
        assert np.array_equal(host.index_of.astype(np.int64)[owned], ref["index_of"][owned]) and (host.index_of[~owned] == dev.CLUMP_NONE).all(), (what, "twin")
        assert R.same_bits(host.r2, ref["r2"]) and host.n_clumps == ref["n_clumps"], (what, "twin")
    return ref


def not_vacuous(ref):
    """The issue's condition, on the ORACLE's result alone."""
    assert sum(1 for s in R.sizes(ref) if s >= 2) >= 20, R.sizes(ref)
    assert ref["unassigned"] >= 1 and ref["claimed_before_turn"] >= 1


# ---- samples ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_sample_counts(dev, kind):
    dm = matrix(dev, kind)
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 130, 200):
        ref = clump_and_check(dev, dm, kind, BASE, ("samples", n, kind), n_samples=n, twin=n in (1, 17, 65))
        if n >= 15:
            not_vacuous(ref)
        if n == 1:
            assert ref["n_clumps"] == ref["candidates"] and (ref["index_of"] >= 0).sum() == ref["candidates"]   # one sample: every r^2 is NaN


@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_sample_lists(dev, kind):
    dm = matrix(dev, kind)
    not_vacuous(clump_and_check(dev, dm, kind, BASE, "every second sample", samples=list(range(0, SAMPLES, 2))))
    not_vacuous(clump_and_check(dev, dm, kind, BASE, "the late half", samples=list(range(70, SAMPLES))))      # starts inside the second vector
    clump_and_check(dev, dm, kind, BASE, "the first sample only", samples=[0])
    clump_and_check(dev, dm, kind, BASE, "the last sample only", samples=[SAMPLES - 1])
    clump_and_check(dev, dm, kind, BASE, "two far samples", samples=[3, SAMPLES - 2])


# ---- participants, candidates, windows ---------------------------------------------------------------------------------------------------------
def candidate_p(rows, mode, seed):
    """p over `rows` rows, every row a participant at p2 = 0.5 (no NaN), candidates at p1 = 0.01 by `mode`; tied values among both."""
    rng = np.random.default_rng(seed)
    p = 0.02 + rng.integers(0, 40, size=rows) / 100.0
    low = rng.integers(0, 4, size=rows) / 400.0                                      # 0, 0.0025, 0.005, 0.0075: ties and p = 0
    if mode == "one":
        p[rows // 2] = 0.0
    elif mode == "third":
        p[::3] = low[::3]
    elif mode == "all":
        p = low
    return p


@pytest.mark.parametrize("kind", ["complete", "missing"])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 129, 300])
def test_participants_candidates_windows(dev, kind, rows):
    dm = matrix(dev, kind)
    claimed = 0
    for mode in ("none", "one", "third", "all"):
        p = candidate_p(rows, mode, rows)
        for window in (0, 4, 2**32 - 1):
            if rows == 300 and mode == "all" and window > 4:
                continue                                                             # 90 000 pairs in the oracle: 129 rows cover three tiles already
            prm = R.params(p1=0.01, p2=0.5, r2=0.3, window=window)
            ref = clump_and_check(dev, dm, kind, prm, (rows, mode, window, kind), n_samples=21, row_count=rows, p=np.concatenate([p, np.ones(ROWS - rows)]),
                                  twin=rows in (65, 129))
            assert ref["participants"] == rows and (ref["candidates"] == 0) == (mode == "none")
            claimed += int((ref["index_of"] >= 0).sum()) - ref["n_clumps"]
    if rows >= 63:
        assert claimed > 0


def test_row_range_keep_mask_and_no_positions(dev):
    kind = "missing"
    dm = matrix(dev, kind)
    keep = np.random.default_rng(8).random(250) >= 1 / 3
    not_vacuous(clump_and_check(dev, dm, kind, BASE, "range", n_samples=77, row_begin=37, row_count=250))
    masked = clump_and_check(dev, dm, kind, R.params(p1=0.05, p2=0.12, r2=0.3, window=90), "range and keep mask", n_samples=77, row_begin=37, row_count=250, keep=keep)
    assert sum(1 for s in R.sizes(masked) if s >= 2) >= 10
    clump_and_check(dev, dm, kind, BASE, "no kept row", row_begin=37, row_count=250, keep=np.zeros(250, dtype=bool))
    clump_and_check(dev, dm, kind, BASE, "an empty range", row_begin=ROWS, row_count=0)
    clump_and_check(dev, dm, kind, R.params(p1=0.03, p2=0.1, r2=0.3, window=40), "rows as positions", n_samples=77, pos=None)
    clump_and_check(dev, dm, kind, BASE, "every p NaN", p=np.full(ROWS, np.nan))


# ---- thresholds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_thresholds(dev, kind):
    dm = matrix(dev, kind)
    _, _, d, pos, p = cohort(kind)
    first = p.copy()
    first[0], first[1], first[2] = 0.0, 0.05, 0.05                                    # row 0 is the first index; its duplicate and complement take part
    for r2 in (0.0, 0.3, 1.0):
        ref = clump_and_check(dev, dm, kind, R.params(p1=0.03, p2=0.1, r2=r2, window=90), ("r2", r2, kind), n_samples=130, p=first)
        assert ref["index_of"][:3].tolist() == [0, 0, 0] and ref["r2"][:3].tolist() == [1.0, 1.0, 1.0]
        if r2 == 0.0:
            assert ref["unassigned"] <= 3                                             # every defined pair in the window is claimed
        if r2 == 1.0:
            assert (ref["index_of"] == 0).sum() == 3


# ---- both cores, every matrix kind, row tables on and off -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_matrix_kinds(dev, fmh_opts, kind, row_hi):
    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    _, called, d, _, _ = cohort(kind)
    if kind != "complete":
        assert (d == R.NOT_CALLED).any()
    for planes in (True, False):
        dm = matrix(dev, kind, planes=planes)
        not_vacuous(clump_and_check(dev, dm, kind, BASE, (kind, planes, row_hi), n_samples=130, twin=planes))


# ---- chunks, grids, a caller's stream --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_launch_variety(dev, kind):
    import torch

    from ferromic_amd import _abi

    dm = matrix(dev, kind)
    wide = R.params(p1=0.06, p2=0.12, r2=0.3, window=2**32 - 1)                       # every participant is in every candidate's window
    ref = clump_and_check(dev, dm, kind, wide, "one chunk", n_samples=40)
    tile = 32 if kind == "missing" else 64
    tiles, partner_tiles = -(-ref["candidates"] // tile), -(-ref["participants"] // 64)
    assert tiles >= 3 and partner_tiles >= 4
    with _abi.options(FMH_CLUMP_BUDGET_BYTES=partner_tiles * tile * 8):             # one candidate tile per launch: `tiles` chunks
        clump_and_check(dev, dm, kind, wide, "a chunk per candidate tile", n_samples=40, twin=False)
        not_vacuous(clump_and_check(dev, dm, kind, BASE, "chunks of the banded request", n_samples=40, twin=False))
    with _abi.options(FMH_CLUMP_BUDGET_BYTES=partner_tiles * tile * 8 - 1):
        with pytest.raises(_abi.FerromicHipError, match="bytes of scratch, above FMH_CLUMP_BUDGET_BYTES") as err:
            clump_and_check(dev, dm, kind, wide, "a budget below one candidate tile", n_samples=40, twin=False)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED
    with _abi.options(FMH_CLUMP_HOST_BYTES=ref["candidates"] * partner_tiles * 8 - 1):
        with pytest.raises(_abi.FerromicHipError, match="bytes on the host, above FMH_CLUMP_HOST_BYTES") as err:
            clump_and_check(dev, dm, kind, wide, "a host budget one byte short", n_samples=40, twin=False)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED
    with _abi.options(FMH_CLUMP_HOST_BYTES=ref["candidates"] * partner_tiles * 8):
        clump_and_check(dev, dm, kind, wide, "the host budget to the byte", n_samples=40, twin=False)
    for blocks in (1, 3, 4096):
        with _abi.options(FMH_GRID_BLOCKS=blocks):
            clump_and_check(dev, dm, kind, wide, ("FMH_GRID_BLOCKS", blocks), n_samples=40, twin=False)
            clump_and_check(dev, dm, kind, BASE, ("FMH_GRID_BLOCKS", blocks, "banded"), n_samples=40, twin=False)
    own = torch.cuda.Stream()
    handle = C.c_void_p(own.cuda_stream)
    assert bool(handle.value), "a stream of its own, not the NULL stream"
    clump_and_check(dev, dm, kind, BASE, "a caller's stream", n_samples=40, twin=False, stream=handle)


# ---- pairs -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_pairs(dev, kind):
    dm = matrix(dev, kind)
    _, _, d, _, _ = cohort(kind)
    rng = np.random.default_rng(4)
    for P in (0, 1, 63, 64, 65):
        a, b = rng.integers(0, ROWS, size=P), rng.integers(0, ROWS, size=P)
        if P:
            a[0], b[0] = 0, ROWS - 1                                                  # rows far apart
        if P > 4:
            a[1], b[1] = 7, 7                                                         # a == b
            a[2], b[2] = 0, 1                                                         # the duplicate
            a[3], b[3] = 2, 0                                                         # the complement
            a[4], b[4] = ROWS - 1, 5                                                  # a monomorphic row
        for samples in (None, list(range(5, SAMPLES, 3))):
            cols = np.arange(SAMPLES) if samples is None else np.asarray(samples)
            got = dev.geno_ld_pairs(dm, a, b, samples=samples)
            want = R.pair_counts(d[:, cols], a, b)
            assert got.shape == (P, 6) and np.array_equal(got, want), (P, kind, samples is None)
            assert np.array_equal(got, dev.geno_ld_pairs_host(d[:, cols], a, b))
            r2 = dev.geno_ld_r2(got)
            assert R.same_bits(r2, [R.r2_of(c) for c in want])
            if P > 4:
                assert r2[1] in (1.0,) or np.isnan(r2[1])
                assert r2[2] == 1.0 and r2[3] == 1.0 and np.isnan(r2[4])
    n17 = dev.geno_ld_pairs(dm, [0, 9], [3, 250], n_samples=17)
    assert np.array_equal(n17, R.pair_counts(d[:, :17], [0, 9], [3, 250]))


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------
def assert_clumps(c, ref, rel, rows, positions, p, what):
    """A Clumps against the oracle's result over the kept rows `rel` of `rows` rows in play."""
    index_rows = [int(rel[i]) for i in ref["indexes"]]
    assert len(c) == ref["n_clumps"] and c.index_rows.dtype == np.int64 and c.index_rows.tolist() == index_rows, what
    assert R.same_bits(c.index_p, [p[r] for r in index_rows]) and c.sizes.tolist() == R.sizes(ref), what
    want_index, want_r2 = np.full(rows, -1, dtype=np.int64), np.full(rows, np.nan)
    owned = ref["index_of"] >= 0
    want_index[rel[owned]] = rel[ref["index_of"][owned]]
    want_r2[rel] = ref["r2"]
    assert c.index_of.dtype == np.int64 and np.array_equal(c.index_of, want_index) and R.same_bits(c.r2, want_r2), what
    number = {r: k for k, r in enumerate(index_rows)}
    assert c.clump_of.tolist() == [number.get(int(i), -1) for i in want_index], what
    assert np.array_equal(c.positions, positions) and np.array_equal(c.index_mask(), want_index == np.arange(rows)), what
    for k in (0, len(c) - 1):
        assert c.members(k).tolist() == np.flatnonzero(want_index == index_rows[k]).tolist(), what
    assert repr(c) == "Clumps(clumps=%d, rows=%d, assigned=%d)" % (ref["n_clumps"], rows, int(owned.sum())), what


def test_python_surface(fm):
    x, called, d, pos, p = cohort("missing", seed=2, samples=24)
    positions = pos + 1000
    geno = np.where(called, x, -1).astype(np.int8).reshape(ROWS, 24, 2)
    whole = [0, 2, 3, 5, 8, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20, 21, 22, 23]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(1, 0)]
    pop = fm.Population.from_numpy("p", geno, positions, haps, int(positions[-1]) + 1)
    ref = R.clump(d[:, whole], positions, p, BASE)
    assert sum(1 for s in R.sizes(ref) if s >= 2) >= 10
    assert_clumps(pop.ld_clump(p, **BASE), ref, np.arange(ROWS), ROWS, positions, p, "Population.ld_clump")
    sites = np.arange(ROWS) % 5 != 2
    rel = np.flatnonzero(sites)
    assert_clumps(pop.ld_clump(p, sites=sites, **BASE), R.clump(d[rel][:, whole], positions[rel], p[rel], BASE), rel, ROWS, positions, p, "Population.ld_clump(sites)")
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = [dict(position=int(positions[i]), genotypes=[None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(24)])
                for i in range(ROWS)]
    samples = [1, 2, 5, 10, 11, 12, 17, 20, 23]
    assert_clumps(fm.ld_clump(variants, p, samples=samples, **BASE), R.clump(d[:, samples], positions, p, BASE), np.arange(ROWS), ROWS, positions, p, "ld_clump(samples)")
    assert_clumps(fm.ld_clump(variants, p, **BASE), R.clump(d, positions, p, BASE), np.arange(ROWS), ROWS, positions, p, "ld_clump")
    a, b = [0, 0, 2, 40, ROWS - 1], [0, 1, 0, 250, 17]
    r2, counts = fm.genotype_ld(variants, a, b, samples=samples, counts=True)
    want = R.pair_counts(d[:, samples], a, b)
    assert counts.dtype == np.int64 and np.array_equal(counts, want) and R.same_bits(r2, [R.r2_of(c) for c in want])
    assert R.same_bits(fm.genotype_ld(variants, a, b), [R.r2_of(c) for c in R.pair_counts(d, a, b)])


def test_scan_clump_score_round_trip(fm):
    """association_scan -> ld_clump -> polygenic_score on a tiny cohort: the score over the clumps' index sites is the score over the oracle's."""
    x, called, d, pos, _ = cohort("missing", seed=3, rows=120, samples=40)
    positions = pos + 10
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = [dict(position=int(positions[i]), genotypes=[None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(40)])
                for i in range(120)]
    rng = np.random.default_rng(5)
    g = np.where(d == R.NOT_CALLED, 1, d).astype(np.float64)
    y = g[10] - g[60] + 0.5 * g[100] + rng.normal(0, 0.7, size=40)
    scan = fm.association_scan(variants, y)
    p, beta = scan.p[:, 0], scan.beta[:, 0]
    prm = R.params(p1=0.05, p2=0.5, r2=0.2, window=60)
    ref = R.clump(d, positions, p, prm)
    assert ref["n_clumps"] >= 3 and sum(1 for s in R.sizes(ref) if s >= 2) >= 2
    c = fm.ld_clump(variants, p, **prm)
    assert c.index_rows.tolist() == ref["indexes"]
    mask = np.zeros(120, dtype=bool)
    mask[ref["indexes"]] = True
    got = fm.polygenic_score(variants, np.where(c.index_mask(), np.nan_to_num(beta), 0.0)).score
    want = fm.polygenic_score(variants, np.where(mask, np.nan_to_num(beta), 0.0)).score
    assert np.array_equal(got, want) and np.abs(got).sum() > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_order(dev, fmh_opts):
    """Every refusal of fmh_clump and fmh_geno_ld_pairs that needs a matrix handle; each call but the last of a kind is wrong in a LATER way
    too, so the order shows."""
    from ferromic_amd import _abi

    lib = _abi.load()
    kind = "missing"
    x, called, d, pos, p = cohort(kind)
    dm = matrix(dev, kind)
    ok, bad = dev.clump_params(**BASE), dev.clump_params(p1=0.5, p2=0.1)
    down = np.zeros(ROWS, dtype=np.uint32)
    down[10] = 7
    far = np.ascontiguousarray(p).copy()
    far[20] = 1.5
    index_of = np.zeros(ROWS + 1, dtype=np.uint32)
    samples = np.array([3, 2], dtype=np.uint32)

    def call(m=dm._h, s=None, n=SAMPLES, r0=0, rc=ROWS, x_=None, p_=p, prm=ok, out=index_of):
        return lib.fmh_clump(m, None if s is None else s.ctypes.data, n, r0, rc, None, None if x_ is None else x_.ctypes.data,
                             None if p_ is None else np.ascontiguousarray(p_).ctypes.data, prm, None if out is None else out.ctypes.data, None, None, None)

    cases = [
        (lambda: call(m=None, prm=None, n=0), b"NULL matrix"),
        (lambda: call(prm=None, p_=None, n=0), b"NULL params"),
        (lambda: call(p_=None, out=None, n=0), b"NULL h_p"),
        (lambda: call(out=None, n=0), b"NULL h_index_of"),
        (lambda: call(n=0, s=samples, rc=ROWS + 1), b"n_samples is 0"),
        (lambda: call(n=2, s=samples, rc=ROWS + 1), b"not strictly ascending"),
        (lambda: call(n=SAMPLES + 1, rc=ROWS + 1), b"exceeds the matrix's 200 samples"),
        (lambda: call(rc=ROWS + 1, prm=bad), b"exceed the matrix's 300 variants"),
        (lambda: call(prm=bad, p_=far), b"0 <= p1 <= p2 <= 1"),
        (lambda: call(prm=dev.clump_params(r2=float("nan")), p_=far), b"NaN"),
        (lambda: call(p_=far, x_=down), b"neither NaN nor within [0, 1]"),
        (lambda: call(x_=down), b"descend"),
    ]
    for make, words in cases:
        assert make() == _abi.FMH_ERR_INVALID and words in lib.fmh_last_error(), (words, lib.fmh_last_error())
    rows = np.array([0, ROWS], dtype=np.uint32)
    out = dev.DeviceBuffer(dm.device, 64)

    def pairs(m=dm._h, s=None, n=SAMPLES, a=rows, b=rows, P=2, o=out.ptr):
        return lib.fmh_geno_ld_pairs(m, None if s is None else s.ctypes.data, n, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data, P, o, None)

    for make, words in [(lambda: pairs(m=None, n=0), b"NULL matrix"), (lambda: pairs(n=0, s=samples), b"n_samples is 0"),
                        (lambda: pairs(n=2, s=samples, a=None), b"not strictly ascending"), (lambda: pairs(a=None), b"NULL row list or output"),
                        (lambda: pairs(o=None), b"NULL row list or output"), (lambda: pairs(), b"pair 1 names rows (300, 300)")]:
        assert make() == _abi.FMH_ERR_INVALID and words in lib.fmh_last_error(), (words, lib.fmh_last_error())
    assert pairs(a=None, b=None, P=0, o=None) == _abi.FMH_OK
    # FMH_ERR_UNSUPPORTED: ploidy, no packed image (each wrong in the budget too), the budget
    fmh_opts.setenv("FMH_CLUMP_BUDGET_BYTES", "1")
    haploid = upload(dev, np.ascontiguousarray(x[:, :41]), None, 1, planes=True, ploidy=1)
    assert call(m=haploid._h, n=2) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy 2" in lib.fmh_last_error()
    assert pairs(m=haploid._h, n=2, P=1) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy 2" in lib.fmh_last_error()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    unpacked = upload(dev, np.where(called, x, 0).astype(np.uint8), None, 1, ploidy=2)
    fmh_opts.delenv("FMH_LAYOUT")
    assert call(m=unpacked._h) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
    assert pairs(m=unpacked._h, P=1) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
    assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_CLUMP_BUDGET_BYTES = 1" in lib.fmh_last_error()
    none = np.ones(ROWS)                                                             # no participant: no scratch, whatever the budget
    assert call(p_=none) == _abi.FMH_OK and (index_of[:ROWS] == dev.CLUMP_NONE).all()
    fmh_opts.delenv("FMH_CLUMP_BUDGET_BYTES")
    assert call() == _abi.FMH_OK and (index_of[:ROWS] != dev.CLUMP_NONE).sum() > 40
    unpacked.pack()
    assert call(m=unpacked._h) == _abi.FMH_OK
