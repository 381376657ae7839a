"""The logistic association scan on the device (fmh_assoc_homalt_sums, fmh_logistic_score, ferromic.logistic_scan) against
tests/logistic_ref.py, the oracle written from the definition.  Every sum is compared with array_equal on int64, every f64 bitwise (with
the host twin, and end to end with the oracle), NaN positions equal.  Cohorts and uploads are test_gpu_sfs.py's (random bits under the
uncalled entries of every allele plane), with ploidy 2.  Outputs are pre-filled with 0xA5: a call must write every entry.

The shapes of H are tests/test_gpu_assoc.py's, the smallest at which each part of the contraction can go wrong: samples around a 32-bit word
(15 .. 17), a 128-column vector (63 .. 65), the 256 samples of a staged B chunk (255 .. 257) and several chunks (1 023 .. 1 025, 2 049), in
matrices of n and n + 3 samples; value columns around a B tile (1, 3, 4, 5), a value group (8, 9, 16, 17) and the limit (63, 64); rows around
a 16-row tile, a wave's 32 rows, the 128 rows of a pass and the 4 096 rows of an item, and ranges that begin and end off a 16-row block; the
value limits and the digit edges; the widest row the packed layout takes with every genotype hom-alt.  Preconditions are asserted on the
oracle alone, before the device is called, so that a mask-blind kernel, or one that returns S or C, cannot pass."""

import ctypes as C

import numpy as np
import pytest

from tests import assoc_ref as A
from tests import logistic_ref as R
from tests.concurrent_harness import run_workers
from tests.test_gpu_assoc import COLUMNS, EDGES, LIMIT, ROWS, SAMPLES, WIDE_SAMPLES, values_for
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def preconditions(kind, x, called, values, samples=None):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 64 rows, >= 15 samples)."""
    max_allele, missing = KINDS[kind]
    H = R.homalt_sums(x, called, values, samples)
    S, Cs = A.sums(x, called, values, samples)
    assert len({tuple(r) for r in H.tolist()}) >= 8, "the hom-alt sums differ between rows"
    assert (H != S).any() and (H != Cs).any()
    if missing or max_allele > 1:
        # an uncalled genotype on a hom-alt bit pattern: the lowest allele bit of both entries is 1 (as stored: alleles 1, 3, 5, 7 and whatever
        # lies under a missing entry is random), so a kernel that forgets the mask counts it
        ok = (np.ones(x.shape, dtype=bool) if called is None else np.asarray(called, dtype=bool)) & (x <= 1)
        c = ok[:, 0::2] & ok[:, 1::2]
        both = ((x[:, 0::2] & 1) == 1) & ((x[:, 1::2] & 1) == 1)
        assert (both & ~c).any(), "some uncalled genotype sits on a hom-alt bit pattern"
    return H


def check(dev, dm, x, called, values, what, samples=None, n_samples=None, row_begin=0, row_count=None, stream=None):
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    H = R.homalt_sums(x[row_begin:row_begin + rows], None if called is None else called[row_begin:row_begin + rows], values, sel)
    got = dev.assoc_homalt_sums(dm, values, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, stream=stream, fill=0xA5)
    assert got.dtype == np.int64 and got.shape == H.shape, what
    assert np.array_equal(got, H), (what, "H", np.argwhere(got != H)[:4].tolist())
    return got


# ---- H: shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_samples_around_words_vectors_and_chunks(dev, kind):
    max_allele, missing = KINDS[kind]
    for n in SAMPLES + WIDE_SAMPLES:
        rows = 70 if n >= 1023 else 130
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=31)
            values = values_for(n, 5)
            if n >= 63:
                preconditions(kind, x, called, values, np.arange(n))
            dm = upload(dev, x, called, max_allele, n % 2 == 0, ploidy=2)
            try:
                check(dev, dm, x, called, values, (kind, n, extra), n_samples=n)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_value_columns(dev, kind):
    max_allele, missing = KINDS[kind]
    for n, rows in ((70, 300), (300, 70)):
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=32)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            for k in COLUMNS:
                values = values_for(n, k)
                preconditions(kind, x, called, values)
                check(dev, dm, x, called, values, (kind, n, k))
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_rows_and_ranges(dev, kind):
    max_allele, missing = KINDS[kind]
    n = 34
    values = values_for(n, 5)
    for rows in ROWS:
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=33)
        if rows >= 255:
            preconditions(kind, x, called, values)
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            check(dev, dm, x, called, values, (kind, rows))
            if rows >= 255:   # ranges that begin and end off a 16-row block
                check(dev, dm, x, called, values, (kind, rows, "range"), row_begin=5, row_count=rows - 12)
                check(dev, dm, x, called, values, (kind, rows, "one row"), row_begin=rows - 1, row_count=1)
                check(dev, dm, x, called, values, (kind, rows, "17 rows"), row_begin=15, row_count=17)
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_special_values(dev, kind):
    max_allele, missing = KINDS[kind]
    n, rows = 130, 70
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=34)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for name, fill in (("+2^30", LIMIT), ("-2^30", -LIMIT), ("zeros", 0)):
            check(dev, dm, x, called, np.full((n, 3), fill, dtype=np.int32), (kind, name))
        edges = np.array(EDGES + [e * 65536 for e in EDGES if abs(e * 65536) <= LIMIT] + [-e for e in EDGES], dtype=np.int32)
        values = np.tile(edges, (n, 1))                      # every sample carries every edge: one edge per column
        values[1::2] = np.roll(edges, 1)
        got = check(dev, dm, x, called, values, (kind, "digit edges"))
        assert got.any()
    finally:
        dm.close()


def test_accumulators_at_the_widest_row(dev):
    """Every genotype hom-alt, V = 63 * 2^24 - 128 * 65 793 everywhere: the digits are -128, -128, -128, 63 and a digit accumulator ends at
    -n * 128.  n = 300 000 is the widest row a packed matrix takes (600 000 columns)."""
    n = 300000
    v = 63 * (1 << 24) - 128 * 65793
    assert A.digits(v) == [-128, -128, -128, 63]
    x = np.ones((2, 2 * n), dtype=np.uint8)
    values = np.full((n, 1), v, dtype=np.int32)
    dm = dev.DeviceMatrix.from_host(x, None, 2, n, 2, 1)
    try:
        assert dev.assoc_homalt_sums(dm, values, fill=0xA5).tolist() == [[n * v]] * 2
        samples = np.arange(0, n, 2, dtype=np.uint32)          # and a list over the whole width
        assert dev.assoc_homalt_sums(dm, values[: samples.size], samples=samples, fill=0xA5).tolist() == [[samples.size * v]] * 2
    finally:
        dm.close()


# ---- H: call arguments -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists(dev, kind):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(35)
    for total, rows in ((68, 130), (300, 130), (1100, 70)):
        x, called = cohort(rows, 2 * total, max_allele, missing, seed=36)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            scattered = np.flatnonzero(rng.random(total) < 0.3)
            lists = {"every second": np.arange(0, total, 2), "tail": np.arange(total - 9, total), "one": np.array([total // 2]),
                     "first": np.array([0]), "scattered": scattered, "identity": np.arange(total)}
            for name, samples in lists.items():
                values = values_for(samples.size, 4, seed=total)
                if samples.size >= 64:
                    preconditions(kind, x, called, values, samples)
                check(dev, dm, x, called, values, (kind, total, name), samples=samples)
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_options_streams_and_uploads_change_nothing(dev, fmh_opts, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n, rows = 300, 600
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=37)
    values = values_for(n, 17)
    H = preconditions(kind, x, called, values)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    for row_hi in ("0", "2"):
        fmh_opts.setenv("FMH_ROW_HI", row_hi)      # with and without the tables of the rows that hold upper alleles / uncalled columns
        for planes in (False, True):
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                for item_rows in (16, 48, 4096):
                    for blocks in (1, 3):
                        fmh_opts.setenv("FMH_ASSOC_ITEM_ROWS", str(item_rows))
                        fmh_opts.setenv("FMH_GRID_BLOCKS", str(blocks))
                        got = check(dev, dm, x, called, values, (kind, row_hi, planes, item_rows, blocks))
                        assert np.array_equal(got, H)
                fmh_opts.delenv("FMH_GRID_BLOCKS")
                fmh_opts.setenv("FMH_GRID_PER_CU", "1")
                check(dev, dm, x, called, values, (kind, "one workgroup per CU"), stream=handle)
                fmh_opts.delenv("FMH_GRID_PER_CU")
                fmh_opts.delenv("FMH_ASSOC_ITEM_ROWS")
                check(dev, dm, x, called, values, (kind, "a caller's stream"), stream=handle)
                stream.synchronize()
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_ones_column_equals_genotype_counts(dev, kind):
    """Against code that existed before: with a column of ones H is fmh_genotype_counts' hom_alt track, and fmh_assoc_sums' S - 2 H its het
    track."""
    max_allele, missing = KINDS[kind]
    n, rows = 270, 300
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=38)
    samples = np.flatnonzero(np.random.default_rng(39).random(n) < 0.8)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for sel in (None, samples):
            count = n if sel is None else sel.size
            values = np.ones((count, 2), dtype=np.int32)
            values[:, 1] = -3
            H = dev.assoc_homalt_sums(dm, values, samples=sel, row_begin=7, row_count=rows - 20, fill=0xA5)
            S = dev.assoc_sums(dm, values, samples=sel, row_begin=7, row_count=rows - 20, called=False).dosage
            qc = dev.genotype_counts(dm, samples=sel, row_begin=7, row_count=rows - 20, sample=())
            alt, het = qc.site["hom_alt"].astype(np.int64), qc.site["het"].astype(np.int64)
            assert alt.any() and het.any()
            assert np.array_equal(H, np.stack([alt, -3 * alt], axis=1))
            assert np.array_equal(S - 2 * H, np.stack([het, -3 * het], axis=1))
    finally:
        dm.close()


def test_refusals_leave_no_launch_error(dev):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    values = values_for(16, 3)
    out = dev.DeviceBuffer(dm.device, 8 * 40 * 64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    too_large, too_small = values.copy(), values.copy()
    too_large[5, 1], too_small[7, 2] = LIMIT + 1, -LIMIT - 1

    def call(m=dm, samples=None, n=8, r0=0, rc=40, v=values, k=3, h=out.ptr):
        return lib.fmh_assoc_homalt_sums(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if v is None else p(v), k,
                                         h, None)

    # fmh_logistic_score: S, C [rows][K], H [rows][Pb], three tracks, T, e, c, Pb, two outputs
    rows, c, Pb = 5, 1, 2
    K = Pb * (c + 3)
    bufs = [dev.DeviceBuffer.from_numpy(dm.device, np.zeros(rows * K, dtype=np.int64)) for _ in range(3)]
    trk = dev.DeviceBuffer.from_numpy(dm.device, np.ones(rows, dtype=np.uint32))
    res = [dev.DeviceBuffer(dm.device, 8 * rows * Pb) for _ in range(2)]
    total, e = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int32)
    good = [bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, trk.ptr, trk.ptr, trk.ptr, rows, p(total), p(e), c, Pb, res[0].ptr, res[1].ptr, dm.device, None]

    def score(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.fmh_logistic_score(*args)

    hip = C.CDLL("libamdhip64.so")   # the runtime the library is linked against: already mapped, so this cannot fail where the test runs
    try:
        assert call() == 0
        # fmh_assoc_sums' order: NULL matrix, values, output; n_samples; K; a value; the sample list; the row range; ploidy; no packed image
        invalid = [call(m=None), call(v=None), call(h=None), call(n=0), call(n=(1 << 21) + 1), call(k=0), call(k=65), call(v=too_large),
                   call(v=too_small), call(n=9), call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2), call(samples=u32(4, 2), n=2),
                   call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(m=None, v=None) == _abi.FMH_ERR_INVALID and b"matrix" in lib.fmh_last_error()
        assert call(v=None, h=None, n=0) == _abi.FMH_ERR_INVALID and b"values" in lib.fmh_last_error()
        assert call(n=(1 << 21) + 1, k=0) == _abi.FMH_ERR_INVALID and b"2^21" in lib.fmh_last_error()
        assert call(v=too_large, n=9) == _abi.FMH_ERR_INVALID and b"2^30" in lib.fmh_last_error()
        assert call(n=9, r0=41) == _abi.FMH_ERR_INVALID and b"matrix's 8 samples" in lib.fmh_last_error()
        assert call(m=haploid, n=4, r0=41) == _abi.FMH_ERR_INVALID and b"rows" in lib.fmh_last_error()
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        assert call(rc=0) == 0 and call(r0=40, rc=0) == 0
        assert score() == 0
        bad = [score(**{f"a{i}": None}) for i in (0, 1, 2, 3, 4, 5, 7, 8, 11, 12)] + [score(a10=0), score(a10=17), score(a9=62)]
        assert bad == [_abi.FMH_ERR_INVALID] * len(bad), bad
        assert score(a6=0) == 0 and score(a6=0, a0=None, a11=None) == 0       # no rows: nothing is read
        assert hip.hipGetLastError() == 0
        edge = values.copy()
        edge[5, 1], edge[7, 2] = LIMIT, -LIMIT
        check(dev, dm, x, called, edge[:8], "after the refusals")
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- fmh_logistic_score against its host twin -------------------------------------------------------------------------------------------------
def score_inputs(dev, c_in, rows=4097):
    """A cohort whose first rows are crafted, the library's null model of the largest phenotype batch that fits, and numpy's sums."""
    n = 400 if c_in == 61 else 150
    rng = np.random.default_rng(70 + c_in)
    x = (rng.random((rows, 2 * n)) < rng.uniform(0.05, 0.9, size=(rows, 1))).astype(np.uint8)
    called = rng.random((rows, 2 * n)) > 0.05
    if rows > 8:
        x[0] = 0                       # monomorphic reference
        x[1] = 1                       # monomorphic alternative
        called[2] = False              # N = 0
        x[3, 0::2], x[3, 1::2] = 0, 1  # all het
        called[3] = True
    B = 64 // (c_in + 3)
    cov = rng.normal(size=(n, c_in)) if c_in else None
    y = (rng.random((n, B)) < 0.4).astype(np.float64)
    model = dev.logistic_null(y, cov)
    assert model.n_basis == c_in and model.fitted.all() and model.batch == B and len(model.values) == 1
    v = model.values[0]
    S, Cs = A.sums(x, called, v)
    H = R.homalt_sums(x, called, v[:, c_in + 2::c_in + 3])
    if rows > 8:   # a negative variance: nothing of w on the called genotypes, everything called
        S, Cs = S.copy(), Cs.copy()
        for p in range(B):
            kw = p * (c_in + 3) + c_in + 2
            S[5, kw], H[5, p], Cs[5, kw] = 0, 0, model.total[p, c_in + 2]
    return S, Cs, H, A.tracks(x, called), model


@pytest.mark.parametrize("c_in", [0, 1, 5, 61])
def test_score_equals_host_twin(dev, c_in):
    S, Cs, H, trk, model = score_inputs(dev, c_in)
    W, B = c_in + 3, model.batch
    for Pb in sorted({1, min(2, B), B}):
        total, e = model.total[:Pb].reshape(-1), model.exponent[:Pb].reshape(-1)
        for rows in (1, 255, 256, 257, 4097):
            at = 6 if rows == 1 else 0    # a single row: one that carries a test
            args = (S[at:at + rows, :Pb * W], Cs[at:at + rows, :Pb * W], H[at:at + rows, :Pb], *[t[at:at + rows] for t in trk], total, e, c_in)
            U_ref, V_ref = dev.logistic_score_host(*args)
            U, V = dev.logistic_score(0, *args, fill=0xA5)
            what = (c_in, Pb, rows)
            assert R.same_f64(U, U_ref) and R.same_f64(V, V_ref), what
            if rows > 8:
                assert np.isnan(U_ref[:3]).all() and np.isnan(V_ref[:3]).all() and np.isfinite(U_ref[3:]).all() and np.isfinite(V_ref[3:]).all(), what
                assert (V_ref[5] < 0.0).all() and (V_ref[6:] > 0.0).mean() > 0.99, what
            else:
                assert np.isfinite(U_ref).all() and (V_ref > 0.0).all(), what
    if c_in in (0, 5):     # the oracle's loop once per shape of the model, on the rows that matter
        U_o, V_o = R.score(S[:40, :W], Cs[:40, :W], H[:40, :1], *[t[:40] for t in trk], model.total[0].tolist(), model.exponent[0], c_in)
        U, V = dev.logistic_score(0, S[:40, :W], Cs[:40, :W], H[:40, :1], *[t[:40] for t in trk], model.total[0], model.exponent[0], c_in, fill=0xA5)
        assert R.same_f64(U, U_o) and R.same_f64(V, V_o)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def phenotypes_for(n, cov, P, seed, g_planted):
    """P case / control phenotypes: the first carries the planted effect, the second depends on a covariate, phenotype 6 is separated by one."""
    rng = np.random.default_rng(seed)
    eta = np.full((n, P), -0.4)
    eta[:, 0] += 1.6 * (g_planted - g_planted.mean())
    eta[:, 1] += 0.5 * cov[:, 0]
    y = (rng.random((n, P)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    if P > 6:
        y[:, 6] = (cov[:, 1] > 0.0).astype(np.float64)
    return y


def assert_scan(scan, x, called, y, cov, samples, positions, planted, what):
    ref = R.scan(x, called, y, cov, samples)
    model = ref["model"]
    expect = np.ones(y.shape[1], dtype=bool)
    if y.shape[1] > 6:
        expect[6] = False
    assert model["fitted"].tolist() == expect.tolist(), (what, model["reason"])     # the oracle first
    if planted is not None:
        assert np.nanargmin(ref["p"][:, 0]) == planted, what
    for name in ("score", "variance", "chi2", "z", "p", "beta", "se"):
        got = getattr(scan, name)
        assert got.shape == ref[name].shape and R.same_f64(got, ref[name]), (what, name)
        assert np.isnan(got[:, ~expect]).all() and np.isfinite(got[:, expect]).any(axis=0).all(), (what, name)
    trk = ref["tracks"]
    N = trk[0].astype(np.int64) + trk[1] + trk[2]
    assert np.array_equal(scan.n_called, N.astype(np.uint32)), what
    with np.errstate(invalid="ignore", divide="ignore"):
        assert R.same_f64(scan.alt_frequency, (trk[1].astype(np.float64) + 2.0 * trk[2]) / (2.0 * N)), what
    assert np.array_equal(scan.positions, positions) and len(scan) == x.shape[0], what
    assert np.array_equal(scan.fitted, model["fitted"]) and np.array_equal(scan.iterations, model["iterations"]), what
    assert np.array_equal(scan.n_cases, model["n_cases"]) and np.array_equal(scan.reason, model["reason"]), what
    assert np.array_equal(scan.covariates_dropped, np.flatnonzero(model["dropped"])), what
    assert np.array_equal(scan.covariates_kept, np.flatnonzero(~model["dropped"])), what


def test_population_logistic_scan(fm, fmh_opts):
    """300 sites x 140 diploid samples with missing calls; the population holds both haplotypes of 120 samples and one of three more.  c = 5
    and P = 9: two phenotype batches (8 + 1); a small budget: several row chunks; phenotype 6 is separated and comes back unfitted."""
    rng = np.random.default_rng(51)
    x, called = cohort(300, 280, 1, True, seed=51)
    x = x.copy()
    x[17] = (rng.random(280) < 0.45).astype(np.uint8)           # the planted row: common, and called everywhere
    called = called.copy()
    called[17] = True
    geno = np.where(called, x, -1).astype(np.int8).reshape(300, 140, 2)
    whole = sorted(int(s) for s in rng.choice(140, size=120, replace=False))
    halves = [s for s in range(140) if s not in whole][:3]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(s, 1) for s in halves]
    positions = np.arange(300, dtype=np.int64) * 7
    pop = fm.Population.from_numpy("p", geno, positions, haps, 3000)
    _, g = A.genotypes(x, called, whole)
    cov = rng.normal(size=(120, 5))
    y = phenotypes_for(120, cov, 9, 52, g[17])
    scan = pop.logistic_scan(y, cov)
    assert isinstance(scan, fm.LogisticScan)
    assert_scan(scan, x, called, y, cov, whole, positions, 17, "Population.logistic_scan")
    assert "LogisticScan(samples=120, sites=300, phenotypes=9, fitted=8, covariates=5)" == repr(scan)
    # a budget small enough to force three chunks: (2 K + 3 Pb) * 8 bytes per row with K = 64, Pb = 8
    fmh_opts.setenv("FMH_ASSOC_BUDGET_BYTES", str((2 * 64 + 3 * 8) * 8 * 128))
    assert_scan(pop.logistic_scan(y, cov), x, called, y, cov, whole, positions, 17, "three chunks")
    fmh_opts.reset()
    one = pop.logistic_scan(y[:, 0])                             # a single phenotype as [n], no covariates
    assert_scan(one, x, called, y[:, :1], None, whole, positions, 17, "one phenotype")
    for bad in (y[:119], np.full((120, 1), 0.5), np.full((120, 1), np.nan)):
        with pytest.raises(ValueError):
            pop.logistic_scan(bad)
    with pytest.raises(ValueError):
        pop.logistic_scan(y, cov[:40])


def test_logistic_scan_of_variant_records(fm):
    """A sparse variant list (records with missing genotypes), a region that cuts rows off both ends, a sample list."""
    rng = np.random.default_rng(61)
    x, called = cohort(60, 160, 1, True, seed=61)
    x, called = x.copy(), called.copy()
    x[20] = (rng.random(160) < 0.5).astype(np.uint8)
    called[20] = True
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(80)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    positions = 100 + 10 * np.arange(60, dtype=np.int64)
    _, g = A.genotypes(x, eff_called)
    cov = rng.normal(size=(80, 2))
    y = phenotypes_for(80, cov, 2, 62, g[20])
    assert_scan(fm.logistic_scan(variants, y, cov), x, eff_called, y, cov, None, positions, 20, "logistic_scan")
    samples = list(range(1, 80, 2)) + [78]
    samples = sorted(set(samples))
    ys, covs = y[samples], cov[samples]
    assert_scan(fm.logistic_scan(variants, ys, covs, samples=samples), x, eff_called, ys, covs, samples, positions, None, "logistic_scan(samples)")
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    assert_scan(fm.logistic_scan(variants, y, cov, region=region), x[6:52], eff_called[6:52], y, cov, None, positions[6:52], 14,
                "logistic_scan(region)")
    for bad in ([2, 1], [0, 0], [80], [-1]):
        with pytest.raises(ValueError):
            fm.logistic_scan(variants, y[:2], samples=bad)
    with pytest.raises(ValueError):
        fm.logistic_scan(variants, y[:5])
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(80)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.logistic_scan(haploid, y)


# ---- concurrency -----------------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(dev):
    """Two host threads, each on a stream of its own, call the two new device entry points at once: the integers and the bits are the
    single-threaded ones."""
    import torch

    max_allele, missing = KINDS["multi3-missing"]
    n, rows = 300, 2000
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=81)
    values = values_for(n, 17)
    H = preconditions("multi3-missing", x, called, values)
    S, Cs, Hs, trk, model = score_inputs(dev, 5)
    args = (S, Cs, Hs, *trk, model.total.reshape(-1), model.exponent.reshape(-1), 5)
    U_ref, V_ref = dev.logistic_score_host(*args)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    streams = [torch.cuda.Stream() for _ in range(2)]
    handles = [C.c_void_p(s.cuda_stream) for s in streams]
    try:
        single = dev.assoc_homalt_sums(dm, values, fill=0xA5)
        assert np.array_equal(single, H)

        def check_h(got):
            assert np.array_equal(got, H)

        def check_score(got):
            assert R.same_f64(got[0], U_ref) and R.same_f64(got[1], V_ref)

        workers = [("homalt", lambda: dev.assoc_homalt_sums(dm, values, stream=handles[0], fill=0xA5), check_h),
                   ("score", lambda: dev.logistic_score(0, *args, stream=handles[1], fill=0xA5), check_score)]
        run_workers(workers, rounds=3, timeout_s=120.0).assert_ok()
        for s in streams:
            s.synchronize()
    finally:
        dm.close()
