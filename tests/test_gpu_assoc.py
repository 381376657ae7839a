"""The association scan on the device (fmh_assoc_sums, ferromic.association_scan) against tests/assoc_ref.py, the oracle written from the
definition.  Every sum is compared with array_equal on int64, every f64 of the end-to-end scan bitwise with the oracle, NaN positions
equal.  Cohorts and uploads are test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2.  Outputs
are pre-filled with 0xA5: the call must write every entry.

Shapes are the smallest at which each part of the kernel can go wrong:
  * samples around a 32-bit word = one lane's operand (15 .. 17), one MFMA's contraction = a 128-column vector (63 .. 65), the 256 samples of
    a staged B chunk (255 .. 257), several chunks (1 023 .. 1 025, 2 049), in matrices of n and of n + 3 samples;
  * value columns around a B tile of 16 digit columns (1, 3, 4, 5), a value group of 16 columns (8, 9, 16, 17) and the limit (63, 64);
  * rows around a 16-row MFMA tile, a wave's 32 rows, the 128 rows of a pass and the 4 096 rows of an item, and ranges that begin and end off a
    16-row block;
  * values over the full range, all +2^30, all -2^30, zeros, and the digit edges 127, 128, -128, -129, 32 767, 32 768, -32 769 and those of
    their multiples of 2^16 that stay within +-2^30 (the first four);
  * the accumulator limit: every genotype hom-alt and three digits -128 at the widest row the packed layout takes (600 000 columns = 300 000
    samples; the definition's 2^22 samples do not fit a packed matrix, so a digit accumulator ends at -76 800 000, not at -2^30).
Preconditions are asserted on the oracle alone, before the device is called, so that a transposed, mask-blind or digit-blind kernel cannot
pass."""

import ctypes as C

import numpy as np
import pytest

from tests import assoc_ref as R
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257]
WIDE_SAMPLES = [1023, 1024, 1025, 2049]   # about 70 rows there
COLUMNS = [1, 3, 4, 5, 8, 9, 16, 17, 63, 64]
ROWS = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097]
EDGES = [127, 128, -128, -129, 32767, 32768, -32769]
LIMIT = 1 << 30


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def values_for(n, k, seed=0):
    """[n][k] int32 over the full range; the first entries are the limits and the digit edges (as many as fit)."""
    rng = np.random.default_rng(7 * n + k + seed)
    v = rng.integers(-LIMIT, LIMIT + 1, size=(n, k), dtype=np.int64)
    special = [LIMIT, -LIMIT, 0] + EDGES + [e * 65536 for e in EDGES if abs(e * 65536) <= LIMIT]
    flat = v.reshape(-1)
    flat[: min(flat.size, len(special))] = special[: min(flat.size, len(special))]
    return v.astype(np.int32)


def preconditions(kind, x, called, values, samples=None):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 64 rows, >= 15 samples and >= 3 columns)."""
    max_allele, missing = KINDS[kind]
    S, Cs = R.sums(x, called, values, samples)
    total = np.asarray(values, dtype=np.int64).sum(axis=0)
    assert len({tuple(r) for r in S.tolist()}) >= 8, "the dosage sums differ between rows"
    assert len({tuple(c) for c in S.T.tolist()}) == S.shape[1], "and between columns"
    if missing or max_allele > 1:
        assert (Cs != total).any(axis=1).any(), "some row has an uncalled genotype"
        assert (Cs != S).any()
    d = np.array([R.digits(v) for v in np.asarray(values).reshape(-1)[:4096]])
    assert (d != 0).any(axis=0).all() and (d < 0).any(), "every digit is used and a negative carry occurs"
    return S, Cs


def check(dev, dm, x, called, values, what, samples=None, n_samples=None, row_begin=0, row_count=None, want_called=True, stream=None):
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    S, Cs = R.sums(x[row_begin:row_begin + rows], None if called is None else called[row_begin:row_begin + rows], values, sel)
    got = dev.assoc_sums(dm, values, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, called=want_called, stream=stream,
                         fill=0xA5)
    assert got.dosage.dtype == np.int64 and got.dosage.shape == S.shape, what
    assert np.array_equal(got.dosage, S), (what, "S", np.argwhere(got.dosage != S)[:4].tolist())
    if want_called:
        assert np.array_equal(got.called, Cs), (what, "C", np.argwhere(got.called != Cs)[:4].tolist())
    else:
        assert got.called is None
    return got


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_samples_around_words_vectors_and_chunks(dev, kind):
    max_allele, missing = KINDS[kind]
    for n in SAMPLES + WIDE_SAMPLES:
        rows = 70 if n >= 1023 else 130
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=31)
            values = values_for(n, 5)
            if n >= 15:
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
                if k >= 3:
                    preconditions(kind, x, called, values)
                check(dev, dm, x, called, values, (kind, n, k))
                check(dev, dm, x, called, values, (kind, n, k, "S only"), want_called=False)
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
        assert {tuple(R.digits(v)) for v in edges} >= {(127, 0, 0, 0), (-128, 1, 0, 0), (-128, 0, 0, 0), (127, -1, 0, 0), (-1, -128, 1, 0)}
        check(dev, dm, x, called, values, (kind, "digit edges"))
    finally:
        dm.close()


def test_accumulators_at_the_widest_row(dev):
    """Every genotype hom-alt, V = 63 * 2^24 - 128 * 65 793 everywhere: the digits are -128, -128, -128, 63 and a digit accumulator ends at
    -2 * n * 128.  n = 300 000 is the widest row a packed matrix takes (600 000 columns)."""
    n = 300000
    v = 63 * (1 << 24) - 128 * 65793
    assert R.digits(v) == [-128, -128, -128, 63]
    x = np.ones((2, 2 * n), dtype=np.uint8)
    values = np.full((n, 1), v, dtype=np.int32)
    dm = dev.DeviceMatrix.from_host(x, None, 2, n, 2, 1)
    try:
        got = dev.assoc_sums(dm, values, fill=0xA5)
        assert got.dosage.tolist() == [[2 * n * v]] * 2 and got.called.tolist() == [[n * v]] * 2
        samples = np.arange(0, n, 2, dtype=np.uint32)          # and a list over the whole width
        got = dev.assoc_sums(dm, values[: samples.size], samples=samples, fill=0xA5)
        assert got.dosage.tolist() == [[2 * samples.size * v]] * 2 and got.called.tolist() == [[samples.size * v]] * 2
    finally:
        dm.close()


# ---- call arguments --------------------------------------------------------------------------------------------------------------------
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
                if samples.size >= 15:
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
    S, Cs = preconditions(kind, x, called, values)
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
                        assert np.array_equal(got.dosage, S) and np.array_equal(got.called, Cs)
                fmh_opts.delenv("FMH_GRID_BLOCKS")
                fmh_opts.setenv("FMH_GRID_PER_CU", "1")
                check(dev, dm, x, called, values, (kind, "one workgroup per CU"), stream=handle)
                fmh_opts.delenv("FMH_GRID_PER_CU")
                fmh_opts.delenv("FMH_ASSOC_ITEM_ROWS")
                check(dev, dm, x, called, values, (kind, "a caller's stream"), stream=handle, want_called=False)
                stream.synchronize()
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_ones_column_equals_genotype_counts(dev, kind):
    """An independent device path: with a value column of ones, S = het + 2 hom_alt and C = hom_ref + het + hom_alt of fmh_genotype_counts."""
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
            got = dev.assoc_sums(dm, values, samples=sel, row_begin=7, row_count=rows - 20, fill=0xA5)
            qc = dev.genotype_counts(dm, samples=sel, row_begin=7, row_count=rows - 20, sample=())
            alt = qc.site["het"].astype(np.int64) + 2 * qc.site["hom_alt"].astype(np.int64)
            N = qc.site["hom_ref"].astype(np.int64) + qc.site["het"] + qc.site["hom_alt"]
            assert np.array_equal(got.dosage, np.stack([alt, -3 * alt], axis=1))
            assert np.array_equal(got.called, np.stack([N, -3 * N], axis=1))
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
    out = [dev.DeviceBuffer(dm.device, 8 * 40 * 64) for _ in range(2)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    too_large, too_small = values.copy(), values.copy()
    too_large[5, 1], too_small[7, 2] = LIMIT + 1, -LIMIT - 1

    def call(m=dm, samples=None, n=8, r0=0, rc=40, v=values, k=3, s=out[0].ptr, c=out[1].ptr):
        return lib.fmh_assoc_sums(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if v is None else p(v), k, s, c,
                                  None)

    hip = C.CDLL("libamdhip64.so")   # the runtime the library is linked against: already mapped, so this cannot fail where the test runs
    try:
        assert call() == 0
        # the header's order: NULL matrix, values, d_dosage_sum; n_samples; K; a value; the sample list; the row range; ploidy; no packed image
        invalid = [call(m=None), call(v=None), call(s=None), call(n=0), call(n=(1 << 22) + 1), call(k=0), call(k=65), call(v=too_large),
                   call(v=too_small), call(n=9), call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2), call(samples=u32(4, 2), n=2),
                   call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        assert call(rc=0) == 0 and call(r0=40, rc=0) == 0
        assert hip.hipGetLastError() == 0
        # n = 2^22 + 1 is refused for its own reason, not as "more than the matrix's 8 samples" (which n = 9 is)
        assert call(n=(1 << 22) + 1) == _abi.FMH_ERR_INVALID and b"2^22" in lib.fmh_last_error()
        assert call(n=9) == _abi.FMH_ERR_INVALID and b"2^22" not in lib.fmh_last_error() and b"matrix's 8 samples" in lib.fmh_last_error()
        # the limits themselves are taken, the called sums may be NULL, and the next call is correct
        assert call(c=None) == 0
        edge = values.copy()
        edge[5, 1], edge[7, 2] = LIMIT, -LIMIT
        check(dev, dm, x, called, edge[:8], "after the refusals")
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def model(n, c_in, seed, g_planted):
    """Two phenotypes (the first carries the planted effect) and c_in covariates, the last a copy of the first when there are five."""
    rng = np.random.default_rng(seed)
    cov = rng.normal(size=(n, c_in)) * 4.0 + 2.0 if c_in else None
    if c_in == 5:
        cov[:, 4] = cov[:, 0] * 2.0 - 1.0      # collinear with the first (and the intercept)
    y = rng.normal(size=(n, 2)) + 5.0
    y[:, 0] += 1.5 * g_planted
    if c_in:
        y[:, 1] += 0.4 * cov[:, 0]
    return y, cov


def assert_scan(scan, x, called, y, cov, samples, positions, planted, what):
    n = y.shape[0]
    prep = R.prepare(y, cov)
    S, Cs = R.sums(x, called, prep["values"], samples)
    trk = R.tracks(x, called, samples)
    ref = R.stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"])
    if planted is not None:   # the oracle first
        assert np.nanargmin(ref["p"][:, 0]) == planted, what
    for name in ("beta", "se", "t", "p"):
        got = getattr(scan, name)
        assert got.shape == ref[name].shape and R.same_f64(got, ref[name]), (what, name)
    N = trk[0].astype(np.int64) + trk[1] + trk[2]
    assert np.array_equal(scan.n_called, N.astype(np.uint32)), what
    with np.errstate(invalid="ignore", divide="ignore"):
        assert R.same_f64(scan.alt_frequency, (trk[1].astype(np.float64) + 2.0 * trk[2]) / (2.0 * N)), what
    assert np.array_equal(scan.positions, positions), what
    assert scan.df == n - prep["n_basis"] - 2 and len(scan) == x.shape[0], what
    assert np.array_equal(scan.covariates_dropped, np.flatnonzero(prep["dropped"])), what
    assert np.array_equal(scan.covariates_kept, np.flatnonzero(~prep["dropped"])), what
    if planted is not None:
        assert np.nanargmin(scan.p[:, 0]) == planted, what


def test_population_association_scan(fm, fmh_opts):
    """300 sites x 60 diploid samples with missing calls; the population holds both haplotypes of 44 samples and one of three more."""
    rng = np.random.default_rng(51)
    x, called = cohort(300, 120, 1, True, seed=51)
    x = x.copy()
    x[17] = (rng.random(120) < 0.45).astype(np.uint8)           # the planted row: common, and called everywhere
    called = called.copy()
    called[17] = True
    geno = np.where(called, x, -1).astype(np.int8).reshape(300, 60, 2)
    whole = sorted(int(s) for s in rng.choice(60, size=44, replace=False))
    halves = [s for s in range(60) if s not in whole][:3]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(s, 1) for s in halves]
    positions = np.arange(300, dtype=np.int64) * 7
    pop = fm.Population.from_numpy("p", geno, positions, haps, 3000)
    _, g = R.genotypes(x, called, whole)
    for c_in in (0, 1, 5):
        y, cov = model(44, c_in, 52 + c_in, g[17])
        scan = pop.association_scan(y, cov)
        assert isinstance(scan, fm.AssociationScan)
        assert_scan(scan, x, called, y, cov, whole, positions, 17, ("Population.association_scan", c_in))
        if c_in == 5:
            assert scan.covariates_dropped.tolist() == [4] and scan.df == 44 - 4 - 2
    # a budget small enough to force three chunks: 2 * K * 8 bytes per row, K = 4 + 2
    fmh_opts.setenv("FMH_ASSOC_BUDGET_BYTES", str(2 * 6 * 8 * 128))
    assert_scan(pop.association_scan(y, cov), x, called, y, cov, whole, positions, 17, "three chunks")
    fmh_opts.reset()
    one = pop.association_scan(y[:, 0])                          # a single phenotype as [n]
    assert one.p.shape == (300, 1) and "AssociationScan(samples=44, sites=300, phenotypes=1, covariates=0, df=42)" == repr(one)
    for bad in (y[:43], np.full((44, 1), np.nan)):
        with pytest.raises(ValueError):
            pop.association_scan(bad)
    with pytest.raises(ValueError):
        pop.association_scan(y, cov[:40])


def test_association_scan_of_variant_records(fm):
    """A sparse variant list (records with missing genotypes), a region that cuts rows off both ends, a sample list."""
    rng = np.random.default_rng(61)
    x, called = cohort(60, 48, 1, True, seed=61)
    x, called = x.copy(), called.copy()
    x[20] = (rng.random(48) < 0.5).astype(np.uint8)
    called[20] = True
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(24)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    positions = 100 + 10 * np.arange(60, dtype=np.int64)
    _, g = R.genotypes(x, eff_called)
    y, cov = model(24, 1, 62, g[20])
    assert_scan(fm.association_scan(variants, y, cov), x, eff_called, y, cov, None, positions, 20, "association_scan")
    samples = [1, 2, 5, 7, 8, 10, 11, 13, 17, 20, 21, 23]
    ys, covs = y[samples], cov[samples]
    assert_scan(fm.association_scan(variants, ys, covs, samples=samples), x, eff_called, ys, covs, samples, positions, None, "association_scan(samples)")
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    assert_scan(fm.association_scan(variants, y, cov, region=region), x[6:52], eff_called[6:52], y, cov, None, positions[6:52], 14,
                "association_scan(region)")
    for bad in ([2, 1], [0, 0], [24], [-1]):
        with pytest.raises(ValueError):
            fm.association_scan(variants, y[:2], samples=bad)
    with pytest.raises(ValueError):
        fm.association_scan(variants, y[:5])
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(24)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.association_scan(haploid, y)
