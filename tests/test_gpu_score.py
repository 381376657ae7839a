"""The polygenic score on the device (fmh_score_sums, ferromic.polygenic_score) against tests/score_ref.py, the oracle written from the
definition.  Every sum is compared with array_equal on int64, every f64 of the end-to-end score bitwise with the oracle.  Cohorts and uploads
are test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2; the value ranges and digit edges are
test_gpu_assoc.py's values_for.  Outputs are pre-filled with 0xA5: the call must write every entry.

Shapes are the smallest at which each part of the kernels can go wrong:
  * rows around a lane's 16-row chunk (1, 15 .. 17), one MFMA step (63 .. 65), an item of 64 and of 128 rows (127 .. 129, 257: the reduce
    kernel adds 2 to 5 slabs) and the default item (4 095 .. 4 097), and ranges that begin and end off a 64-row step;
  * samples around a word = tile (1, 2, 15 .. 17), a wave's 64 (63 .. 65), a workgroup's 256 (255 .. 257) and several groups (1 023 .. 1 025),
    in matrices of n and of n + 3 samples; ascending sample lists with gaps, one of which leaves whole tiles and a whole group empty;
  * value columns around a group of 16 (1, 3, 4, 5, 15, 16, 17) and the limit (63, 64), U present and absent, U != V;
  * values over the full range, all +2^30, all -2^30, zeros and the digit edges;
  * the accumulator limit: one item of 2^18 rows, every genotype hom-alt, three digits -128: a digit accumulator ends at -2 * 2^18 * 128.
Preconditions are asserted on the oracle alone, before the device is called, so that a transposed, mask-blind, digit-blind or reduce-less
kernel cannot pass."""

import ctypes as C

import numpy as np
import pytest

from tests import score_ref as R
from tests.test_gpu_assoc import EDGES, LIMIT, values_for
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
COLUMNS = [1, 3, 4, 5, 15, 16, 17, 63, 64]
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def preconditions(kind, x, called, V, U, samples=None):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 64 rows, >= 15 samples and >= 3 columns)."""
    max_allele, missing = KINDS[kind]
    S, Cs = R.sums(x, called, V, U, samples)
    assert len({tuple(r) for r in S.tolist()}) >= min(8, S.shape[0]), "the dosage sums differ between samples"
    assert len({tuple(c) for c in S.T.tolist()}) == S.shape[1], "and between columns"
    if U is not None:
        assert not np.array_equal(np.asarray(U), np.asarray(V)), "a kernel that feeds one digit buffer to both operands fails"
        if missing or max_allele > 1:
            total = np.asarray(U, dtype=np.int64).sum(axis=0)
            assert ((Cs != total).any(axis=1) & (Cs != S).any(axis=1)).any(), "some sample has an uncalled genotype"
    d = R.digit_planes(np.asarray(V).reshape(-1)[:4096])
    assert (d != 0).any(axis=1).all() and (d < 0).any(), "every digit is used and a negative carry occurs"
    return S, Cs


def check(dev, dm, x, called, V, U, what, samples=None, n_samples=None, row_begin=0, row_count=None, stream=None):
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    span = slice(row_begin, row_begin + rows)
    S, Cs = R.sums(x[span], None if called is None else called[span], V, U, sel)
    got = dev.score_sums(dm, V, U, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, stream=stream, fill=FILL)
    assert got.dosage.dtype == np.int64 and got.dosage.shape == S.shape, what
    assert np.array_equal(got.dosage, S), (what, "S", np.argwhere(got.dosage != S)[:4].tolist())
    if U is not None:
        assert np.array_equal(got.called, Cs), (what, "C", np.argwhere(got.called != Cs)[:4].tolist())
    else:
        assert got.called is None
    return got


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_rows_steps_items_and_ranges(dev, fmh_opts, kind):
    max_allele, missing = KINDS[kind]
    n = 34
    plan = [(0, [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097]), (64, [127, 128, 129, 257]), (128, [127, 128, 129, 257]), (100, [129])]
    for item_rows, sizes in plan:   # an item of 100 rows is rounded up to 128
        if item_rows:
            fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", str(item_rows))
        else:
            fmh_opts.delenv("FMH_SCORE_ITEM_ROWS")
        for rows in sizes:
            x, called = cohort(rows, 2 * n, max_allele, missing, seed=71)
            V, U = values_for(rows, 5), values_for(rows, 5, seed=1)
            if rows >= 127:
                preconditions(kind, x, called, V, U)
            dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
            try:
                check(dev, dm, x, called, V, U, (kind, item_rows, rows))
                if rows >= 127:   # ranges that begin and end off a 64-row step: the rows next to them add nothing
                    check(dev, dm, x, called, V[5:rows - 7], U[5:rows - 7], (kind, item_rows, rows, "range"), row_begin=5, row_count=rows - 12)
                    check(dev, dm, x, called, V[:1], U[:1], (kind, item_rows, rows, "one row"), row_begin=rows - 1, row_count=1)
                    check(dev, dm, x, called, V[:65], None, (kind, item_rows, rows, "65 rows"), row_begin=60, row_count=65)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_samples_around_tiles_waves_and_groups(dev, fmh_opts, kind):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", "64")
    rows = 70
    V, U = values_for(rows, 5), values_for(rows, 5, seed=1)
    for n in SAMPLES:
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=72)
            if n >= 15:
                preconditions(kind, x, called, V, U, np.arange(n))
            dm = upload(dev, x, called, max_allele, n % 2 == 0, ploidy=2)
            try:
                check(dev, dm, x, called, V, U, (kind, n, extra), n_samples=n)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists(dev, fmh_opts, kind):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", "64")
    rng = np.random.default_rng(73)
    rows = 130
    V, U = values_for(rows, 4), values_for(rows, 4, seed=1)
    for total in (68, 800):
        x, called = cohort(rows, 2 * total, max_allele, missing, seed=74)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            lists = {"every second": np.arange(0, total, 2), "tail": np.arange(total - 9, total), "one": np.array([total // 2]),
                     "first": np.array([0]), "scattered": np.flatnonzero(rng.random(total) < 0.3), "identity": np.arange(total)}
            if total == 800:   # samples 40 .. 519 are left out: tiles 3 .. 15 of group 0, the whole of group 1, the first tile of group 2
                lists["a tile and a group empty"] = np.concatenate([np.arange(0, 40, 3), np.arange(520, 800, 7)])
            for name, samples in lists.items():
                if samples.size >= 15:
                    preconditions(kind, x, called, V, U, samples)
                check(dev, dm, x, called, V, U, (kind, total, name), samples=samples)
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_value_columns(dev, fmh_opts, kind):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", "64")
    n, rows = 70, 200
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=75)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for k in COLUMNS:
            V, U = values_for(rows, k), values_for(rows, k, seed=1)
            if k >= 3:
                preconditions(kind, x, called, V, U)
            check(dev, dm, x, called, V, U, (kind, k))
            check(dev, dm, x, called, V, None, (kind, k, "S only"))
    finally:
        dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_special_values(dev, kind):
    max_allele, missing = KINDS[kind]
    n, rows = 130, 70
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=76)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for name, fill in (("+2^30", LIMIT), ("-2^30", -LIMIT), ("zeros", 0)):
            check(dev, dm, x, called, np.full((rows, 3), fill, dtype=np.int32), np.full((rows, 3), -fill, dtype=np.int32), (kind, name))
        edges = np.array(EDGES + [e * 65536 for e in EDGES if abs(e * 65536) <= LIMIT] + [-e for e in EDGES], dtype=np.int32)
        V = np.tile(edges, (rows, 1))                        # every row carries every edge: one edge per column
        V[1::2] = np.roll(edges, 1)
        assert {tuple(R.digits(v)) for v in edges} >= {(127, 0, 0, 0), (-128, 1, 0, 0), (-128, 0, 0, 0), (127, -1, 0, 0), (-1, -128, 1, 0)}
        check(dev, dm, x, called, V, np.roll(V, 3, axis=1), (kind, "digit edges"))
    finally:
        dm.close()


def test_accumulators_at_the_limit_of_an_item(dev, fmh_opts):
    """One item of 2^18 rows x 17 samples, every genotype hom-alt, V = 63 * 2^24 - 128 * 65 793 everywhere: the digits are -128, -128, -128, 63
    and a digit accumulator ends at -2 * 2^18 * 128."""
    rows, n = 1 << 18, 17
    v = 63 * (1 << 24) - 128 * 65793
    assert R.digits(v) == [-128, -128, -128, 63]
    x = np.ones((rows, 2 * n), dtype=np.uint8)
    V = np.full((rows, 1), v, dtype=np.int32)
    acc = R.item_accumulators(x, None, V, rows)
    assert acc.shape == (1, 4, n, 1) and acc.min() == -2 * rows * 128 and (acc[0, :3] == -2 * rows * 128).all()
    fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", str(rows))
    dm = dev.DeviceMatrix.from_host(x, None, rows, n, 2, 1)
    try:
        got = dev.score_sums(dm, V, -V, fill=FILL)
        assert got.dosage.tolist() == [[2 * rows * v]] * n and got.called.tolist() == [[-rows * v]] * n
    finally:
        dm.close()


# ---- call arguments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_options_streams_and_uploads_change_nothing(dev, fmh_opts, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n, rows = 300, 600
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=77)
    V, U = values_for(rows, 17), values_for(rows, 17, seed=1)
    S, Cs = preconditions(kind, x, called, V, U)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    for row_hi in ("0", "2"):
        fmh_opts.setenv("FMH_ROW_HI", row_hi)      # with and without the tables of the rows that hold upper alleles / uncalled columns
        for planes in (False, True):
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                for item_rows in (64, 192, 4096):
                    for blocks in (1, 3):
                        fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", str(item_rows))
                        fmh_opts.setenv("FMH_GRID_BLOCKS", str(blocks))
                        got = check(dev, dm, x, called, V, U, (kind, row_hi, planes, item_rows, blocks))
                        assert np.array_equal(got.dosage, S) and np.array_equal(got.called, Cs)
                fmh_opts.delenv("FMH_GRID_BLOCKS")
                fmh_opts.setenv("FMH_GRID_PER_CU", "1")
                check(dev, dm, x, called, V, U, (kind, "one workgroup per CU"), stream=handle)
                fmh_opts.delenv("FMH_GRID_PER_CU")
                fmh_opts.delenv("FMH_SCORE_ITEM_ROWS")
                check(dev, dm, x, called, V, None, (kind, "a caller's stream"), stream=handle)
                stream.synchronize()
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_cross_checks_against_genotype_counts_and_assoc_sums(dev, fmh_opts, kind):
    """Independent device paths.  A column of ones gives, per sample, het + 2 hom_alt of fmh_genotype_counts, and C with U = ones its called
    count.  And the bilinear form sum over (r, i) of c g X[i] W[r], through fmh_assoc_sums (contracted over samples, then with W on the host)
    and through fmh_score_sums (contracted over rows, then with X on the host)."""
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_SCORE_ITEM_ROWS", "128")
    n, rows = 270, 300
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=78)
    rng = np.random.default_rng(79)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for sel in (None, np.flatnonzero(rng.random(n) < 0.8)):
            count = n if sel is None else sel.size
            r0, rc = 7, rows - 20
            ones = np.ones((rc, 2), dtype=np.int32)
            ones[:, 1] = -3
            got = dev.score_sums(dm, ones, ones, samples=sel, row_begin=r0, row_count=rc, fill=FILL)
            qc = dev.genotype_counts(dm, samples=sel, row_begin=r0, row_count=rc, site=())
            alt = qc.sample["het"].astype(np.int64) + 2 * qc.sample["hom_alt"].astype(np.int64)
            N = qc.sample["hom_ref"].astype(np.int64) + qc.sample["het"].astype(np.int64) + qc.sample["hom_alt"].astype(np.int64)
            assert alt.max() > alt.min() and np.array_equal(got.dosage, np.stack([alt, -3 * alt], axis=1))
            assert np.array_equal(got.called, np.stack([N, -3 * N], axis=1))
            X = rng.integers(-1000, 1001, size=(count, 3), dtype=np.int32)
            W = rng.integers(-1000, 1001, size=(rc, 3), dtype=np.int32)
            by_rows = dev.assoc_sums(dm, X, samples=sel, row_begin=r0, row_count=rc, called=False).dosage     # [rc][3]
            by_samples = dev.score_sums(dm, W, samples=sel, row_begin=r0, row_count=rc, fill=FILL).dosage      # [count][3]
            form = (by_rows * W.astype(np.int64)).sum(axis=0)
            assert form.all() and np.array_equal(form, (by_samples * X.astype(np.int64)).sum(axis=0))
    finally:
        dm.close()


def test_refusals_leave_no_launch_error(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    V, U = values_for(40, 3), values_for(40, 3, seed=1)
    out = [dev.DeviceBuffer.from_numpy(dm.device, np.full(8 * 16 * 64, FILL, dtype=np.uint8)) for _ in range(2)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    too_large, too_small = V.copy(), U.copy()
    too_large[5, 1], too_small[7, 2] = LIMIT + 1, -LIMIT - 1

    def call(m=dm, samples=None, n=8, r0=0, rc=40, v=V, u=U, k=3, s=out[0].ptr, c=out[1].ptr):
        return lib.fmh_score_sums(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if v is None else p(v),
                                  None if u is None else p(u), k, s, c, None)

    hip = C.CDLL("libamdhip64.so")   # the runtime the library is linked against: already mapped, so this cannot fail where the test runs
    try:
        assert call() == 0
        # the header's order: NULL matrix, values, d_dosage_sum; U without C and the reverse; n_samples; K; row_count; a value; the sample list;
        # the row range; ploidy; no packed image; the budget
        invalid = [call(m=None), call(v=None), call(s=None), call(u=None), call(c=None), call(n=0), call(k=0), call(k=65), call(rc=(1 << 21) + 1),
                   call(v=too_large), call(u=too_small), call(n=9), call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2),
                   call(samples=u32(4, 2), n=2), call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(rc=(1 << 21) + 1) == _abi.FMH_ERR_INVALID and b"2^21" in lib.fmh_last_error()
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_SCORE_BUDGET_BYTES", "1")
        assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_SCORE_BUDGET_BYTES" in lib.fmh_last_error()
        assert call(rc=0) == 0, "nothing is needed for no rows"
        fmh_opts.delenv("FMH_SCORE_BUDGET_BYTES")
        assert hip.hipGetLastError() == 0
        # no rows: zeros are written, to both outputs
        assert call(rc=0) == 0 and call(r0=40, rc=0) == 0
        for buf in out:
            got = buf.to_numpy(np.int64, 16 * 64)
            assert not got[: 8 * 3].any() and (got[8 * 3:].view(np.uint8) == FILL).all()
        # the limits themselves are taken, the called sums may be left out, and the next call is correct
        assert call(u=None, c=None) == 0
        edge = V.copy()
        edge[5, 1], edge[7, 2] = LIMIT, -LIMIT
        check(dev, dm, x, called, edge, U, "after the refusals")
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def assert_score(got, x, called, w, samples, positions, mode, what):
    ref = R.score(x, called, w, samples, mode)
    S, Cs = ref["S"], ref["C"]
    assert len({tuple(r) for r in S.tolist()}) >= 8 and (Cs != np.array(ref["total"])).any() and (Cs != S).any(), "the oracle first"
    assert got.score.shape == ref["score"].shape and R.same_f64(got.score, ref["score"]), what
    assert got.rows_used == ref["rows_used"] and R.same_f64(got.average, ref["score"] / float(2 * ref["rows_used"])), what
    assert np.array_equal(got.n_called, ref["n_called"]) and np.array_equal(got.dosage_sum, ref["dosage_sum"]), what
    assert got.exponents.tolist() == ref["e"] and np.array_equal(got.positions, positions) and got.mode == mode, what
    assert len(got) == ref["score"].shape[0], what


def test_population_polygenic_score(fm, fmh_opts):
    """300 sites x 60 diploid samples with missing calls; the population holds both haplotypes of 44 samples and one of three more."""
    rng = np.random.default_rng(81)
    rows = 300
    x, called = cohort(rows, 120, 1, True, seed=81)
    geno = np.where(called, x, -1).astype(np.int8).reshape(rows, 60, 2)
    whole = sorted(int(s) for s in rng.choice(60, size=44, replace=False))
    halves = [s for s in range(60) if s not in whole][:3]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(s, 1) for s in halves]
    positions = np.arange(rows, dtype=np.int64) * 7
    pop = fm.Population.from_numpy("p", geno, positions, haps, 3000)
    w = rng.normal(size=(rows, 3)) * np.array([1.0, 1e-9, 4e5])
    w[rng.random(rows) < 0.1] = 0.0                              # rows without a weight are not used
    modes = {"mean": {}, "center": dict(center=True), "zero": dict(missing="zero")}
    one_chunk = {}
    for mode, kw in modes.items():
        got = pop.polygenic_score(w, **kw)
        assert isinstance(got, fm.PolygenicScore)
        assert_score(got, x, called, w, whole, positions, mode, ("Population.polygenic_score", mode))
        one_chunk[mode] = got.score
    assert not np.array_equal(one_chunk["mean"], one_chunk["center"]) and not np.array_equal(one_chunk["mean"], one_chunk["zero"])
    # a budget that holds the digits and slabs of 128 rows (two steps, one row block, one group of 256 samples, twice): three chunks
    fmh_opts.setenv("FMH_SCORE_BUDGET_BYTES", str(2 * (2 * 4096 + 256 * 3 * 8)))
    for mode, kw in modes.items():
        got = pop.polygenic_score(w, **kw)
        assert_score(got, x, called, w, whole, positions, mode, ("three chunks", mode))
        assert R.same_f64(got.score, one_chunk[mode])
    fmh_opts.reset()
    one = pop.polygenic_score(w[:, 0])                           # a single weight column as [rows]
    assert one.score.shape == (44, 1) and R.same_f64(one.score, one_chunk["mean"][:, :1])
    assert repr(one) == f"PolygenicScore(samples=44, columns=1, rows_used={one.rows_used}, mode=mean)"
    for bad, kw in ((w[:299], {}), (np.full((rows, 1), np.nan), {}), (w, dict(center=True, missing="zero"))):
        with pytest.raises(ValueError):
            pop.polygenic_score(bad, **kw)


def test_polygenic_score_of_variant_records(fm):
    """A sparse variant list (records with missing genotypes), a region that cuts rows off both ends, a sample list."""
    rng = np.random.default_rng(91)
    x, called = cohort(60, 48, 1, True, seed=91)
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(24)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    positions = 100 + 10 * np.arange(60, dtype=np.int64)
    w = rng.normal(size=(60, 2))
    assert_score(fm.polygenic_score(variants, w), x, eff_called, w, None, positions, "mean", "polygenic_score")
    samples = [1, 2, 5, 7, 8, 10, 11, 13, 17, 20, 21, 23]
    assert_score(fm.polygenic_score(variants, w, samples=samples, center=True), x, eff_called, w, samples, positions, "center", "polygenic_score(samples)")
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    assert_score(fm.polygenic_score(variants, w[6:52], region=region, missing="zero"), x[6:52], eff_called[6:52], w[6:52], None, positions[6:52], "zero",
                 "polygenic_score(region)")
    with pytest.raises(ValueError):
        fm.polygenic_score(variants, w, region=region)           # one weight row per row in play
