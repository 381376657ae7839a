"""LD scores on the device (fmh_ld_scores) against tests/ldscore_ref.py, the oracle written from the definition, and against the host twin
(fmh_ld_scores_host): q, partners and counted with array_equal - the sums are integers, so tiles, the symmetry and the atomic adds leave no
tolerance.  Cohorts are the founder mosaics of the clumping tests (tests/test_gpu_clump.py: neighbouring sites in LD, row 1 a duplicate and
row 2 a complement of row 0, two monomorphic rows), uploaded as bit planes with RANDOM bits under the uncalled entries.  The outputs are
pre-filled with junk by ferromic_amd.device.ld_scores: every entry has to be WRITTEN.

Shapes are the smallest at which the kernel can go wrong: selected sample counts around the 16 samples of a word, the 64 of an MFMA step and
the 128 of a staged slab (one, two and three slabs), the n < 3 rule, sample lists that start late or skip; participant counts around one
16-row MFMA tile and one, two and three 64-row tiles (TM = 64 in both cores) and 300 (five tiles, fifteen items); windows of nothing, a few
sites and everything; both cores and every matrix kind; chunks, grids and a caller's stream."""

import ctypes as C
import math

import numpy as np
import pytest

from tests import clump_ref as R
from tests import ldscore_ref as L
from tests.test_gpu_clump import cohort, matrix
from tests.test_gpu_sfs import KINDS, upload

pytestmark = pytest.mark.gpu

ROWS, SAMPLES, WIDE = 300, 200, 260
EVERYTHING = 2**32 - 1
TM = 64


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


_oracle = {}


def oracle(dosage, x, window, adjust):
    """The oracle's answer, computed once per request and shared."""
    key = (dosage.shape, dosage.tobytes(), None if x is None else np.asarray(x).tobytes(), window, adjust)
    if key not in _oracle:
        _oracle[key] = L.ld_scores(dosage, x, window, adjust)
    return _oracle[key]


def score_and_check(dev, dm, d, own_pos, what, window=90, adjust=True, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, pos="own", twin=False,
                    stream=None, first=None):
    """fmh_ld_scores against the oracle (and the twin) over the same kept rows and samples; returns the oracle's result.  `first(ref)` runs on
    the oracle's result BEFORE the device is called: the non-vacuity conditions."""
    pos = own_pos if isinstance(pos, str) else pos
    count = d.shape[0] - row_begin if row_count is None else row_count
    rel = np.arange(count) if keep is None else np.flatnonzero(np.asarray(keep, dtype=bool))
    cols = np.arange(d.shape[1] if n_samples is None else n_samples) if samples is None else np.asarray(samples)
    dosage = np.ascontiguousarray(d[row_begin + rel][:, cols])
    x = None if pos is None else pos[row_begin + rel] - (pos[row_begin] if count else 0)
    ref = oracle(dosage, rel if pos is None else x, window, adjust)
    if first is not None:
        first(ref)
    want_q, want_partners, want_counted = np.zeros(count, dtype=np.int64), np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    want_q[rel], want_partners[rel], want_counted[rel] = ref["q"], ref["partners"], ref["counted"]
    positions = None
    if pos is not None:
        positions = np.zeros(dm.variants, dtype=np.uint32)
        positions[row_begin:row_begin + count] = pos[row_begin:row_begin + count] - (pos[row_begin] if count else 0)
    got = dev.ld_scores(dm, dev.ldscore_params(window, adjust), samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=row_count, keep=keep,
                        positions=positions, stream=stream)
    assert np.array_equal(got.partners, want_partners), (what, "partners", np.flatnonzero(got.partners != want_partners)[:8])
    assert np.array_equal(got.counted, want_counted), (what, "counted", np.flatnonzero(got.counted != want_counted)[:8])
    assert got.q.dtype == np.int64 and np.array_equal(got.q, want_q), (what, "q", np.flatnonzero(got.q != want_q)[:8])
    if twin:
        host = dev.ld_scores_host(dosage, dev.ldscore_params(window, adjust), x=rel if pos is None else x)
        assert np.array_equal(host.q, ref["q"]) and np.array_equal(host.partners, ref["partners"]) and np.array_equal(host.counted, ref["counted"]), (what, "twin")
    return ref


def check_cohort(dev, dm, kind, what, seed=1, rows=ROWS, cohort_samples=SAMPLES, **kw):
    _, _, d, pos, _ = cohort(kind, seed, rows, cohort_samples)
    return score_and_check(dev, dm, d, pos, what, **kw)


def not_vacuous(ref):
    """The issue's conditions, on the ORACLE's result alone."""
    assert (ref["scores"] >= 3).sum() >= 100, int((ref["scores"] >= 3).sum())
    assert (ref["counted"] == 0).sum() >= 2 and ref["negative_terms"] >= 1000 and (ref["counted"] < ref["partners"]).any()


# ---- the MFMA operand maps, first: asymmetric data, failures by pair ---------------------------------------------------------------------------
def asymmetric_dosages(rows, n, miss):
    """Row i < 64 has dosage (i + s) % 3 at sample s, but (i + s + 1) % 3 at the two samples 2 i and 2 i + 1 that mark the row (the bare
    pattern repeats every third row); later rows are seeded draws at a frequency of their own.  No two rows and no two 16-sample words look
    alike, so a transposed or permuted operand changes single pair terms."""
    s = np.arange(n)
    rng = np.random.default_rng(rows * 1009 + n)
    d = np.zeros((rows, n), dtype=np.uint8)
    for i in range(rows):
        if i < 64:
            d[i] = (i + s) % 3
            d[i, 2 * i:2 * i + 2] = (i + s[2 * i:2 * i + 2] + 1) % 3
        else:
            f = 0.15 + 0.7 * ((i * 37) % 66) / 66.0
            d[i] = (rng.random(n) < f).astype(np.uint8) + (rng.random(n) < f).astype(np.uint8)
    if miss:
        d[(np.arange(rows)[:, None] * 5 + s[None, :] * 3) % 11 == 0] = R.NOT_CALLED
    return d


@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_operand_maps(dev, kind):
    rows, n = 130, 150                                                                # three tiles of rows (two full), two slabs of samples
    d = asymmetric_dosages(rows, n, kind == "missing")
    from tests.ibd_ref import genotypes_from_dosages

    x, called = genotypes_from_dosages(d, 3, high_allele=1, uncalled=kind == "missing")
    dm = upload(dev, x, called if kind == "missing" else None, 1, planes=True, ploidy=2)
    table = L.pair_table(d)
    for adjust in (False, True):
        terms = np.zeros((rows, rows), dtype=np.int64)
        used = np.zeros((rows, rows), dtype=bool)
        for i in range(rows):
            for j in range(rows):
                v = L.term(tuple(int(c) for c in table[i, j]), adjust)
                if v is not None:
                    terms[i, j], used[i, j] = v, True
        assert used.sum() > 0.9 * rows * rows and len(np.unique(terms)) > 1000        # asymmetric: the pair terms differ
        full = dev.ld_scores(dm, dev.ldscore_params(EVERYTHING, adjust))
        for i in range(rows):
            assert full.q[i] == terms[i].sum() and full.counted[i] == used[i].sum(), "row %d of the %s core: its sum over all 130 partners" % (i, kind)
        for j in (5, 17, 70, 129):                                                    # without row j every other row loses exactly its term with j
            keep = np.ones(rows, dtype=bool)
            keep[j] = False
            less = dev.ld_scores(dm, dev.ldscore_params(EVERYTHING, adjust), keep=keep)
            assert less.q[j] == 0 and less.counted[j] == 0 and less.partners[j] == 0
            for i in range(rows):
                if i != j:
                    assert full.q[i] - less.q[i] == terms[i, j] and full.counted[i] - less.counted[i] == used[i, j], \
                        "pair (%d, %d) of the %s core: a transposed or permuted MFMA operand" % (i, j, kind)
    dm.close()


# ---- samples ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_sample_counts(dev, kind):
    dm = matrix(dev, kind, samples=WIDE)
    for n in (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        for adjust in (True, False) if n in (2, 3, 64, 257) else (True,):
            ref = check_cohort(dev, dm, kind, ("samples", n, kind, adjust), cohort_samples=WIDE, n_samples=n, adjust=adjust, twin=n in (3, 65),
                               first=not_vacuous if n >= 63 and adjust else None)
            if n <= 2 and adjust:
                assert (ref["counted"] == 0).all()                                    # the n < 3 rule
        if n == 1:
            assert (ref["counted"] == 0).all()                                        # one sample: every r^2 is NaN
    dm.close()


@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_sample_lists(dev, kind):
    dm = matrix(dev, kind, samples=WIDE)
    check_cohort(dev, dm, kind, "every second sample", cohort_samples=WIDE, samples=list(range(0, WIDE, 2)), first=not_vacuous)
    check_cohort(dev, dm, kind, "the late half", cohort_samples=WIDE, samples=list(range(70, WIDE)), twin=True, first=not_vacuous)   # starts inside the second vector
    check_cohort(dev, dm, kind, "from the third slab on", cohort_samples=WIDE, samples=list(range(257, WIDE)))
    check_cohort(dev, dm, kind, "three far samples", cohort_samples=WIDE, samples=[3, 130, WIDE - 2])
    dm.close()


# ---- participants, windows, positions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
@pytest.mark.parametrize("rows", [1, 2, 15, 16, 17, TM - 1, TM, TM + 1, 2 * TM + 1, 300])
def test_participants_and_windows(dev, kind, rows):
    dm = matrix(dev, kind)
    for window in (0, 6, 90, EVERYTHING):
        for adjust in (True, False):
            check_cohort(dev, dm, kind, (rows, window, adjust, kind), n_samples=21, row_count=rows, window=window, adjust=adjust, twin=rows in (17, TM + 1))
    check_cohort(dev, dm, kind, (rows, "rows as positions"), n_samples=21, row_count=rows, window=6, pos=None, twin=rows == 17)
    dm.close()


def test_row_range_keep_mask_and_no_positions(dev):
    kind = "missing"
    dm = matrix(dev, kind)
    keep = np.random.default_rng(8).random(250) >= 1 / 3
    check_cohort(dev, dm, kind, "whole", twin=True, first=not_vacuous)
    check_cohort(dev, dm, kind, "range", n_samples=77, row_begin=37, row_count=250, twin=True)
    def half_vacuous(ref):
        assert (ref["scores"] >= 3).sum() >= 50

    check_cohort(dev, dm, kind, "range and keep mask", n_samples=77, row_begin=37, row_count=250, keep=keep, twin=True, first=half_vacuous)
    check_cohort(dev, dm, kind, "range, keep mask, rows as positions", n_samples=77, row_begin=37, row_count=250, keep=keep, pos=None, window=40)
    none = dev.ld_scores(dm, dev.ldscore_params(90), row_begin=37, row_count=250, keep=np.zeros(250, dtype=bool))
    assert not none.q.any() and not none.partners.any() and not none.counted.any()
    assert dev.ld_scores(dm, dev.ldscore_params(90), row_begin=ROWS, row_count=0).q.shape == (0,)
    assert dev.ld_scores(dm, dev.ldscore_params(90), want_partners=False).partners is None
    dm.close()


def test_exact_terms(dev):
    """Window 0 on distinct positions scores every polymorphic row exactly 1; the duplicate and the complement of row 0 give it exactly 1 each."""
    for kind in ("complete", "missing"):
        dm = matrix(dev, kind)
        _, _, d, _, _ = cohort(kind)
        got = dev.ld_scores(dm, dev.ldscore_params(0))
        poly = np.array([not math.isnan(R.r2_of(R.counts(d[k], d[k]))) for k in range(ROWS)])
        assert poly.sum() >= 280 and (got.q[poly] == 1 << 40).all() and (got.counted[poly] == 1).all() and (got.partners == 1).all()
        assert not got.q[~poly].any() and not got.counted[~poly].any() and not poly[ROWS - 1] and not poly[ROWS - 2]
        keep = np.zeros(ROWS, dtype=bool)
        keep[:3] = True
        trio = dev.ld_scores(dm, dev.ldscore_params(EVERYTHING), keep=keep)
        assert trio.q[:3].tolist() == [3 << 40] * 3 and trio.counted[:3].tolist() == [3, 3, 3] and not trio.q[3:].any()
        dm.close()


# ---- the device's two LD routes agree on every integer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_consistency_with_genotype_ld_pairs(dev, kind):
    """200 in-window pairs: q recomputed from fmh_geno_ld_pairs' integers (the popcount route) by the oracle's formula equals the difference
    between two fmh_ld_scores calls (the matrix-core route) whose keep masks differ by one row."""
    dm = matrix(dev, kind)
    _, _, d, pos, _ = cohort(kind)
    rng = np.random.default_rng(12)
    positions = (pos - pos[0]).astype(np.uint32)
    full = dev.ld_scores(dm, dev.ldscore_params(90), positions=positions)
    pairs = 0
    for j in rng.choice(ROWS, size=10, replace=False):
        keep = np.ones(ROWS, dtype=bool)
        keep[j] = False
        less = dev.ld_scores(dm, dev.ldscore_params(90), positions=positions, keep=keep)
        near = np.flatnonzero((np.abs(pos - pos[j]) <= 90) & (np.arange(ROWS) != j))
        rows_i = rng.choice(near, size=20, replace=False)
        counts = dev.geno_ld_pairs(dm, rows_i, np.full(20, j))
        for i, c in zip(rows_i, counts):
            v = L.term(tuple(int(k) for k in c), True)
            assert int(full.q[i] - less.q[i]) == (0 if v is None else v) and int(full.counted[i]) - int(less.counted[i]) == (v is not None), (int(i), int(j), c.tolist())
            assert int(full.partners[i]) - int(less.partners[i]) == 1
            pairs += 1
    assert pairs == 200
    dm.close()


# ---- both cores, every matrix kind, row tables on and off -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_matrix_kinds(dev, fmh_opts, kind, row_hi):
    from ferromic_amd import _abi

    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    x, called, d, _, _ = cohort(kind)
    if kind != "complete":
        assert (d == R.NOT_CALLED).any()
    dm = matrix(dev, kind, planes=True)
    check_cohort(dev, dm, kind, (kind, row_hi), n_samples=130, twin=True, first=not_vacuous)
    check_cohort(dev, dm, kind, (kind, row_hi, "no correction"), n_samples=130, adjust=False)
    dm.close()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")                                           # the matrix keeps its u8 rows and gets no packed image
    unpacked = matrix(dev, kind, planes=False)
    fmh_opts.delenv("FMH_LAYOUT")
    with pytest.raises(_abi.FerromicHipError, match="fmh_matrix_pack") as err:
        dev.ld_scores(unpacked, dev.ldscore_params(90))
    assert err.value.status == _abi.FMH_ERR_UNSUPPORTED
    unpacked.pack()
    check_cohort(dev, unpacked, kind, (kind, row_hi, "packed from u8 rows"), n_samples=130)
    unpacked.close()


# ---- chunks, grids, a caller's stream --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing"])
def test_launch_variety(dev, kind):
    import torch

    from ferromic_amd import _abi

    dm = matrix(dev, kind)
    tiles = -(-ROWS // dev.LDSCORE_TILE)
    items = tiles * (tiles + 1) // 2                                                  # every participant in every window: every tile pair
    assert tiles == 5 and items == 15
    check_cohort(dev, dm, kind, "one chunk", n_samples=40, window=EVERYTHING)
    rows_bytes = ROWS * dev.LDSCORE_ROW_BYTES
    for budget, what in ((rows_bytes + items * dev.LDSCORE_ITEM_BYTES, "the whole item table to the byte"), (rows_bytes + dev.LDSCORE_ITEM_BYTES, "an item per launch"),
                         (rows_bytes + 5 * dev.LDSCORE_ITEM_BYTES, "three chunks")):
        with _abi.options(FMH_LDSCORE_BUDGET_BYTES=budget):
            check_cohort(dev, dm, kind, what, n_samples=40, window=EVERYTHING)
            check_cohort(dev, dm, kind, (what, "banded"), n_samples=40)
    with _abi.options(FMH_LDSCORE_BUDGET_BYTES=rows_bytes + dev.LDSCORE_ITEM_BYTES - 1):
        with pytest.raises(_abi.FerromicHipError, match="need %d bytes of scratch, above FMH_LDSCORE_BUDGET_BYTES" % (rows_bytes + dev.LDSCORE_ITEM_BYTES)) as err:
            check_cohort(dev, dm, kind, "a budget one byte short", n_samples=40, window=EVERYTHING)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED
        none = dev.ld_scores(dm, dev.ldscore_params(90), keep=np.zeros(ROWS, dtype=bool))   # no kept row: no scratch, whatever the budget
        assert not none.q.any()
    for blocks in (1, 3, 4096):
        with _abi.options(FMH_GRID_BLOCKS=blocks):
            check_cohort(dev, dm, kind, ("FMH_GRID_BLOCKS", blocks), n_samples=40, window=EVERYTHING)
            check_cohort(dev, dm, kind, ("FMH_GRID_BLOCKS", blocks, "banded"), n_samples=40)
    own = torch.cuda.Stream()
    handle = C.c_void_p(own.cuda_stream)
    assert bool(handle.value), "a stream of its own, not the NULL stream"
    check_cohort(dev, dm, kind, "a caller's stream", n_samples=40, stream=handle)
    dm.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_order(dev, fmh_opts):
    """Every refusal of fmh_ld_scores that needs a matrix handle; each call but the last of a kind is wrong in a LATER way too, so the order shows."""
    from ferromic_amd import _abi

    lib = _abi.load()
    kind = "missing"
    x, called, d, pos, _ = cohort(kind)
    dm = matrix(dev, kind)
    ok, bad = dev.ldscore_params(90), dev.ldscore_params(90)
    bad.flags = 2
    down = np.zeros(ROWS, dtype=np.uint32)
    down[10] = 7
    q, counted = np.zeros(ROWS + 1, dtype=np.int64), np.zeros(ROWS + 1, dtype=np.uint32)
    samples = np.array([3, 2], dtype=np.uint32)

    def call(m=dm._h, s=None, n=SAMPLES, r0=0, rc=ROWS, x_=None, prm=ok, q_=q, c_=counted):
        return lib.fmh_ld_scores(m, None if s is None else s.ctypes.data, n, r0, rc, None, None if x_ is None else x_.ctypes.data, prm,
                                 None if q_ is None else q_.ctypes.data, None, None if c_ is None else c_.ctypes.data, None)

    cases = [
        (lambda: call(m=None, prm=None, n=0), b"NULL matrix"),
        (lambda: call(prm=None, q_=None, n=0), b"NULL params"),
        (lambda: call(q_=None, c_=None, n=0), b"NULL h_q"),
        (lambda: call(c_=None, n=0), b"NULL h_counted"),
        (lambda: call(n=0, s=samples, rc=ROWS + 1), b"n_samples is 0"),
        (lambda: call(n=2, s=samples, rc=ROWS + 1), b"not strictly ascending"),
        (lambda: call(n=SAMPLES + 1, rc=ROWS + 1), b"exceeds the matrix's 200 samples"),
        (lambda: call(rc=ROWS + 1, prm=bad), b"exceed the matrix's 300 variants"),
        (lambda: call(prm=bad, x_=down), b"flags other than 0 or FMH_LDSCORE_ADJUST"),
        (lambda: call(x_=down), b"descend"),
    ]
    for make, words in cases:
        assert make() == _abi.FMH_ERR_INVALID and words in lib.fmh_last_error(), (words, lib.fmh_last_error())
    # FMH_ERR_UNSUPPORTED: ploidy, no packed image (each wrong in the budget too), the budget
    fmh_opts.setenv("FMH_LDSCORE_BUDGET_BYTES", "1")
    haploid = upload(dev, np.ascontiguousarray(x[:, :41]), None, 1, planes=True, ploidy=1)
    assert call(m=haploid._h, n=2) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy 2" in lib.fmh_last_error()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")
    unpacked = upload(dev, np.where(called, x, 0).astype(np.uint8), None, 1, ploidy=2)
    fmh_opts.delenv("FMH_LAYOUT")
    assert call(m=unpacked._h) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
    assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_LDSCORE_BUDGET_BYTES = 1" in lib.fmh_last_error()
    fmh_opts.delenv("FMH_LDSCORE_BUDGET_BYTES")
    assert call() == _abi.FMH_OK and (counted[:ROWS] > 0).sum() > 250
    dm.close()
    # a row with more than 2^22 partners, then more than 2^31 work items (each wrong in the budget too): a long, narrow matrix, rows as positions
    long_rows, half = 5_400_000, (1 << 21) - 1
    tiles = -(-long_rows // TM)
    last = np.minimum((np.arange(tiles, dtype=np.int64) + 1) * TM, long_rows) - 1
    items = int(((np.minimum(last + half + 1, long_rows) - 1) // TM - np.arange(tiles) + 1).sum())
    assert items > 1 << 31 and 2 * half + 1 <= 1 << 22
    long_dm = upload(dev, np.zeros((long_rows, 2), dtype=np.uint8), None, 1, ploidy=2)
    big_q, big_counted = np.zeros(long_rows, dtype=np.int64), np.zeros(long_rows, dtype=np.uint32)
    fmh_opts.setenv("FMH_LDSCORE_BUDGET_BYTES", "1")
    crowded = dev.ldscore_params((1 << 21), True)                                    # 2^22 + 1 partners from row 2^21 on
    assert call(m=long_dm._h, n=1, rc=long_rows, prm=crowded, q_=big_q, c_=big_counted) == _abi.FMH_ERR_UNSUPPORTED
    assert b"row entry 2097152 of the range has 4194305 partners" in lib.fmh_last_error(), lib.fmh_last_error()
    assert call(m=long_dm._h, n=1, rc=long_rows, prm=dev.ldscore_params(half, True), q_=big_q, c_=big_counted) == _abi.FMH_ERR_UNSUPPORTED
    assert b"more than 2^31 work items (%d tile pairs)" % items in lib.fmh_last_error(), lib.fmh_last_error()
    assert call(m=long_dm._h, n=1, rc=long_rows, prm=dev.ldscore_params(3, True), q_=big_q, c_=big_counted) == _abi.FMH_ERR_UNSUPPORTED
    assert b"FMH_LDSCORE_BUDGET_BYTES = 1" in lib.fmh_last_error()
    fmh_opts.delenv("FMH_LDSCORE_BUDGET_BYTES")
    long_dm.close()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------
def assert_scores(s, ref, rel, rows, positions, window, adjusted, n_samples, what):
    """An LdScores against the oracle's result over the kept rows `rel` of `rows` rows in play."""
    want_q, want_partners, want_counted, want_scores = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.uint32), np.zeros(rows, dtype=np.uint32), np.full(rows, np.nan)
    want_q[rel], want_partners[rel], want_counted[rel], want_scores[rel] = ref["q"], ref["partners"], ref["counted"], ref["scores"]
    assert len(s) == rows and s.q.dtype == np.int64 and np.array_equal(s.q, want_q), what
    assert s.partners.dtype == np.uint32 and np.array_equal(s.partners, want_partners) and np.array_equal(s.counted, want_counted), what
    assert s.scores.dtype == np.float64 and R.same_bits(s.scores, want_scores), what
    assert np.array_equal(s.positions, positions) and s.window == window and s.adjusted is adjusted and s.n_samples == n_samples, what
    assert s.m_sites == int(np.isfinite(want_scores).sum()), what
    assert repr(s) == "LdScores(rows=%d, scored=%d, window=%d, adjusted=%s, n_samples=%d)" % (rows, s.m_sites, window, adjusted, n_samples), what


def test_python_surface(fm):
    x, called, d, pos, _ = cohort("missing", seed=2, samples=24)
    positions = pos + 1000
    geno = np.where(called, x, -1).astype(np.int8).reshape(ROWS, 24, 2)
    whole = [0, 2, 3, 5, 8, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20, 21, 22, 23]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(1, 0)]
    pop = fm.Population.from_numpy("p", geno, positions, haps, int(positions[-1]) + 1)
    everything = np.arange(ROWS)
    ref = L.ld_scores(d[:, whole], positions, 90, True)
    assert (ref["scores"] >= 3).sum() >= 50
    assert_scores(pop.ld_scores(window=90), ref, everything, ROWS, positions, 90, True, len(whole), "Population.ld_scores")
    sites = np.arange(ROWS) % 5 != 2
    rel = np.flatnonzero(sites)
    assert_scores(pop.ld_scores(window=40, sites=sites, adjust=False), L.ld_scores(d[rel][:, whole], positions[rel], 40, False), rel, ROWS, positions, 40, False, len(whole),
                  "Population.ld_scores(sites)")
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = [dict(position=int(positions[i]), genotypes=[None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(24)])
                for i in range(ROWS)]
    samples = [1, 2, 5, 10, 11, 12, 17, 20, 23]
    assert_scores(fm.ld_scores(variants, window=90, samples=samples), L.ld_scores(d[:, samples], positions, 90, True), everything, ROWS, positions, 90, True, len(samples),
                  "ld_scores(samples)")
    assert_scores(fm.ld_scores(variants), L.ld_scores(d, positions, 1_000_000, True), everything, ROWS, positions, 1_000_000, True, 24, "ld_scores")
    inside = (positions >= 1100) & (positions < 1300)
    assert_scores(fm.ld_scores(variants, window=30, region=(1100, 1299)), L.ld_scores(d[inside], positions[inside], 30, True), np.arange(int(inside.sum())), int(inside.sum()),
                  positions[inside], 30, True, 24, "ld_scores(region)")


def test_scan_scores_regression_round_trip(fm):
    """association_scan -> t^2 -> ld_scores -> .regression on a tiny cohort, against the oracle's regression on the same arrays."""
    x, called, d, pos, _ = cohort("missing", seed=3, rows=120, samples=40)
    positions = pos + 10
    whole_missing = ~(called[:, 0::2] & called[:, 1::2])
    variants = [dict(position=int(positions[i]), genotypes=[None if whole_missing[i, s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(40)])
                for i in range(120)]
    rng = np.random.default_rng(5)
    g = np.where(d == R.NOT_CALLED, 1, d).astype(np.float64)
    y = g[10] - g[60] + 0.5 * g[100] + rng.normal(0, 0.7, size=40)
    chi2 = fm.association_scan(variants, y).t[:, 0] ** 2
    scores = fm.ld_scores(variants, window=60)
    ref = L.ld_scores(d, positions, 60, True)
    assert np.array_equal(scores.q, ref["q"]) and R.same_bits(scores.scores, ref["scores"]) and scores.m_sites == int(np.isfinite(ref["scores"]).sum()) < 120
    assert np.isnan(chi2).any() and np.isfinite(chi2).sum() >= 100
    for kw in (dict(blocks=10), dict(blocks=5, intercept=1.0)):
        want = L.regress(chi2, ref["scores"], 40, scores.m_sites, kw["blocks"], kw.get("intercept"))
        got = scores.regression(chi2, **kw)
        other = fm.ld_score_regression(chi2, scores.scores, 40, **kw)
        for name in ("h2", "h2_se", "intercept", "intercept_se", "ratio", "mean_chi2", "lambda_gc"):
            assert R.same_bits([getattr(got, name)], [want[name]]) and R.same_bits([getattr(other, name)], [want[name]]), (name, kw)
        assert got.n_used == want["n_used"] and got.blocks == kw["blocks"]
