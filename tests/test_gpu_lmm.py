"""The mixed-model scan's device projections (fmh_lmm_projections) and its Python surface against tests/lmm_ref.py, the oracle written from
the definition.  Cohorts and uploads are test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2.

Tolerance, derived.  u = 2^-53.  A sum of n products in ANY order (the kernel's: four at a time inside an MFMA, 64 samples per stage) is within
(n + 2) u sum |terms| of the exact value, so |T^_k - T_k| <= E_k = (n + 2) u sum_i |basis_ik x_i|.  lin_j = sum_k linear_jk T_k over K terms
that carry that error: |lin^ - lin| <= sum_k |linear_jk| E_k + (K + 2) u sum_k |linear_jk T_k|.  quad_p = sum_k weights_pk T_k^2:
|T^^2 - T^2| <= 2 |T| E + E^2, one more rounding for the square: |quad^ - quad| <= sum_k |weights_pk| (2 |T_k| E_k + E_k^2) + (K + 3) u
sum_k |weights_pk| T_k^2.  The oracle sums in np.longdouble, rounds once and so sits well inside the same bound; the tests assert twice the
bound, as test_gpu_grm.py does, and print the worst error / bound.  The tracks c and a are integers: array_equal.

Shapes are the smallest at which each part can go wrong: samples 1, 2, 15 .. 17 (the word of 16 samples = 4 MFMA K steps), 63 .. 65 (the LDS
stage of 64 samples), 129 and 257 (a third and a fifth stage) in matrices of n and n + 3 samples and under sample lists; K = 1, 15 .. 17 (a
component tile), 64, 65 (the component group of a stage) and n with a NON-symmetric random basis; P = 1 and 16; L = 1, 15 .. 17, 64 (the
coefficient tiles, all four instantiations of the kernel); rows 1, 15 .. 17, 63 .. 65, 255 .. 257 (tile, wave and pass edges), 1 030, and
ranges that start off a 16-row block; FMH_LMM_ITEM_ROWS small enough that 1 030 rows are several items.  Every case runs twice (equal bits).
Preconditions are asserted on the oracle alone, before the device is called, for cohorts of 255 rows and more, so that a class-confused,
mask-blind, transposed or square-blind kernel cannot pass."""

import ctypes as C

import numpy as np
import pytest

from tests import grm_ref
from tests import lmm_ref as R
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 129, 257]
COMPONENTS = [1, 15, 16, 17, 64, 65]
LINEAR = [1, 15, 16, 17, 64]
ROWS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1030]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def coefficients(n, K, P, L, seed):
    """A non-symmetric random basis [n][K], positive weights [P][K] (with zeros among them) and signed linear rows [L][K]."""
    rng = np.random.default_rng(seed * 1000003 + n * 7919 + K * 31 + P + L)
    basis = rng.normal(size=(n, K)) * rng.uniform(0.1, 3.0, size=(1, K))
    weights = rng.uniform(0.0, 2.0, size=(P, K)) * (rng.random((P, K)) < 0.9)
    linear = rng.normal(size=(L, K))
    return basis, weights, linear


def preconditions(kind, code, basis, weights, linear, ref):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 255 rows, three samples or more)."""
    n, K = basis.shape
    c, a = ref["c"], ref["a"]
    if KINDS[kind][1]:
        assert (c == 0).any(), "a row without a called genotype occurs"
    assert ((c > 0) & ((a == 0) | (a == 2 * c))).any(), "a monomorphic row occurs"
    big_q, big_l = 1000 * 2 * ref["quad_bound"], 1000 * 2 * ref["lin_bound"]

    def shows(**wrong):
        other = R.projections(code, basis, weights, linear, **wrong)
        return (np.abs(other["quad"] - ref["quad"]) > big_q).any() or (np.abs(other["lin"] - ref["lin"]) > big_l).any()

    assert shows(swap_hom=True), "hom-ref and hom-alt swapped would show"
    if (code == 3).any():
        assert shows(missing_as_zero=True), "a missing call read as 0 instead of mu would show"
    if K == n and n > 1:
        assert shows(transpose=True), "the basis transposed would show"
    other = R.projections(code, basis, weights, linear, weights_on_t=True)
    assert (np.abs(other["quad"] - ref["quad"]) > big_q).any(), "weights applied to T instead of T^2 would show"


def check(dev, dm, x, called, what, basis, weights, linear, samples=None, n_samples=None, row_begin=0, row_count=None, stream=None, ref=None, pre=False):
    """One device call (twice) against the oracle; `pre`: assert the preconditions first (what[0] is the cohort's kind).  Returns the device's result."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    code = grm_ref.codes(x[row_begin : row_begin + rows], None if called is None else called[row_begin : row_begin + rows], sel)
    if ref is None:
        ref = R.projections(code, basis, weights, linear)
    if pre:
        preconditions(what[0], code, basis, weights, linear, ref)
    kw = dict(samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, stream=stream)
    got = dev.lmm_projections(dm, basis, weights, linear, fill=np.nan, **kw)
    again = dev.lmm_projections(dm, basis, weights, linear, fill=-7.0, **kw)
    assert np.array_equal(got.called, ref["c"]) and np.array_equal(got.allele_count, ref["a"]), what
    assert not np.isnan(got.quad).any() and not np.isnan(got.lin).any(), (what, "every entry is written")
    wq, wl = R.worst_ratio(got.quad, ref["quad"], ref["quad_bound"]), R.worst_ratio(got.lin, ref["lin"], ref["lin_bound"])
    print(f"lmm {what}: worst err / (2 bound): quad {wq:.3e}, lin {wl:.3e}")
    assert wq <= 1.0 and wl <= 1.0, (what, wq, wl)
    assert np.array_equal(got.quad.view(np.uint64), again.quad.view(np.uint64)) and np.array_equal(got.lin.view(np.uint64), again.lin.view(np.uint64)), what
    return got


# ---- samples: word, MFMA-step and stage edges, both upload forms, K = n ---------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_sample_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    rows = 257
    for at, n in enumerate(SAMPLES):
        P, L = (1, 16)[at % 2], LINEAR[at % len(LINEAR)]
        basis, weights, linear = coefficients(n, n, P, L, seed=1)
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=5)
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                check(dev, dm, x, called, (kind, planes, n, extra, P, L), basis, weights, linear, n_samples=n, pre=n >= 3)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists_and_component_counts(dev, kind):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7)
    for total in (3, 68, 260):  # a partial word; 65 + 3 samples cross a stage; a list over five stages
        x, called = cohort(300, 2 * total, max_allele, missing, seed=26)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            gaps = np.flatnonzero(rng.random(total) < 0.6)
            if gaps.size == 0:
                gaps = np.array([total - 1])
            lists = {"none": None, "all": np.arange(total), "gaps": gaps, "last-two": np.arange(max(total - 2, 0), total)}
            for at, (name, samples) in enumerate(lists.items()):
                n = total if samples is None else len(samples)
                for K in (COMPONENTS[(at + total) % len(COMPONENTS)], COMPONENTS[(at + total + 3) % len(COMPONENTS)]):
                    basis, weights, linear = coefficients(n, K, 16 if K % 2 else 1, LINEAR[(at + K) % len(LINEAR)], seed=2)
                    check(dev, dm, x, called, (kind, total, name, K), basis, weights, linear, samples=samples, pre=n >= 3)
            if total == 68:
                basis, weights, linear = coefficients(65, 65, 1, 17, seed=3)
                check(dev, dm, x, called, (kind, total, "first 65"), basis, weights, linear, n_samples=65, pre=True)
        finally:
            dm.close()


# ---- rows: tile, wave and pass edges; ranges that start off a 16-row block --------------------------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rows_and_ranges(dev, fmh_opts, kind, row_hi):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    n = 20
    for at, rows in enumerate(ROWS):
        K, L, P = COMPONENTS[at % len(COMPONENTS)], LINEAR[at % len(LINEAR)], (16, 1)[at % 2]
        basis, weights, linear = coefficients(n, K, P, L, seed=4)
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=8)
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            check(dev, dm, x, called, (kind, row_hi, rows, K, P, L), basis, weights, linear, pre=rows >= 255)
            if rows > 2:
                r0, rc = rows // 3, rows - rows // 3 - 1  # 1 030: rows [343, 1 029)
                check(dev, dm, x, called, (kind, row_hi, rows, "range"), basis, weights, linear, row_begin=r0, row_count=rc)
            if rows > 20:
                check(dev, dm, x, called, (kind, row_hi, rows, "range from 5"), basis, weights, linear, row_begin=5, row_count=17)
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_item_and_grid_sizes_change_no_bit(dev, fmh_opts, kind):
    """1 030 rows as 1, 4 and 9 items on 1, 3 and the default number of workgroups: a workgroup takes several items, an item several passes,
    the last item and the last pass are short."""
    max_allele, missing = KINDS[kind]
    n = 70
    x, called = cohort(1030, 2 * n, max_allele, missing, seed=9)
    basis, weights, linear = coefficients(n, 65, 16, 17, seed=5)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        first = check(dev, dm, x, called, (kind, "default"), basis, weights, linear, pre=True)
        for item_rows in ("128", "300", "4096"):
            for blocks in (None, "1", "3"):
                fmh_opts.setenv("FMH_LMM_ITEM_ROWS", item_rows)
                if blocks is not None:
                    fmh_opts.setenv("FMH_GRID_BLOCKS", blocks)
                got = dev.lmm_projections(dm, basis, weights, linear, fill=np.nan)
                fmh_opts.reset()
                assert np.array_equal(got.quad.view(np.uint64), first.quad.view(np.uint64)), (item_rows, blocks)
                assert np.array_equal(got.lin.view(np.uint64), first.lin.view(np.uint64)), (item_rows, blocks)
        fmh_opts.setenv("FMH_GRID_PER_CU", "1")
        got = dev.lmm_projections(dm, basis, weights, linear, fill=np.nan, row_begin=7, row_count=1000)
        fmh_opts.reset()
        ref = dev.lmm_projections(dm, basis, weights, linear, fill=np.nan, row_begin=7, row_count=1000)
        assert np.array_equal(got.quad.view(np.uint64), ref.quad.view(np.uint64)) and np.array_equal(got.lin.view(np.uint64), ref.lin.view(np.uint64))
        # a row's sums do not depend on where its range starts
        assert np.array_equal(ref.quad.view(np.uint64), first.quad[7:1007].view(np.uint64)) and np.array_equal(ref.lin.view(np.uint64), first.lin[7:1007].view(np.uint64))
    finally:
        dm.close()


# ---- calling conventions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_runs_on_a_stream_and_tracks_are_genotype_counts(dev, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n = 70
    x, called = cohort(300, 2 * n, max_allele, missing, seed=10)
    basis, weights, linear = coefficients(n, n, 1, 2, seed=6)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        on_stream = check(dev, dm, x, called, (kind, "on a stream"), basis, weights, linear, stream=handle, pre=True)
        plain = check(dev, dm, x, called, (kind, "NULL stream"), basis, weights, linear)
        assert np.array_equal(on_stream.quad.view(np.uint64), plain.quad.view(np.uint64)) and np.array_equal(on_stream.lin.view(np.uint64), plain.lin.view(np.uint64))
        qc = dev.genotype_counts(dm, sample=None).site
        assert np.array_equal(plain.called, qc["hom_ref"] + qc["het"] + qc["hom_alt"]) and np.array_equal(plain.allele_count, qc["het"] + 2 * qc["hom_alt"])
        stream.synchronize()
    finally:
        dm.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_leave_no_launch_error(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    basis, weights, linear = coefficients(8, 8, 2, 3, seed=7)
    bufs = [dev.DeviceBuffer.from_numpy(dm.device, a) for a in (basis, weights, linear)]
    out_q, out_l = dev.DeviceBuffer.from_numpy(dm.device, np.zeros(40 * 2)), dev.DeviceBuffer.from_numpy(dm.device, np.zeros(40 * 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u32 = lambda *v: np.array(v, dtype=np.uint32)

    def call(m=dm, samples=None, n=8, r0=0, rc=40, b=bufs[0].ptr, K=8, w=bufs[1].ptr, P=2, l=bufs[2].ptr, L=3, q=out_q.ptr, o=out_l.ptr):
        return lib.fmh_lmm_projections(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, b, K, w, P, l, L, q, o, None, None, None)

    try:
        invalid = [call(m=None), call(b=None), call(w=None), call(l=None), call(q=None), call(o=None), call(n=0), call(n=9), call(samples=u32(0, 8), n=2),
                   call(samples=u32(3, 3), n=2), call(samples=u32(4, 2), n=2), call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41), call(K=0),
                   call(K=32769), call(P=0), call(P=17), call(L=0), call(L=65)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=haploid, n=99) == _abi.FMH_ERR_INVALID             # the order: the samples,
        assert call(m=haploid, n=4, r0=41) == _abi.FMH_ERR_INVALID       # the rows
        assert call(m=haploid, n=4, K=0) == _abi.FMH_ERR_INVALID         # and the limits before the ploidy,
        assert call(m=unpacked, L=65) == _abi.FMH_ERR_INVALID            # the limits before the packed image,
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_PCA_BUDGET_BYTES", "1000")
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()  # the packed image before the budget
        assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_PCA_BUDGET_BYTES" in lib.fmh_last_error()
        fmh_opts.reset()
        assert call(rc=0) == 0 and call(r0=40, rc=0) == 0
        assert not out_q.to_numpy(np.float64, 80).any() and not out_l.to_numpy(np.float64, 120).any(), "a refused call wrote nothing"
        check(dev, dm, x, called, "after the refusals", basis, weights, linear)
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- through `import ferromic` ------------------------------------------------------------------------------------------------------------------------
def close(got, want, what):
    """The CPU test's tolerance: 1e-6 of max(1, |reference|), NaN in the same places."""
    ok = np.isfinite(want)
    assert np.array_equal(ok, np.isfinite(got)), what
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-6 * np.maximum(1.0, np.abs(want[ok]))), what


def test_python_surface_end_to_end(fm, fmh_opts):
    variants, samples = 600, 120
    code = R.related_codes(variants, samples, seed=31, missing=0.02)
    x = np.zeros((variants, 2 * samples), dtype=np.uint8)
    x[:, 0::2], x[:, 1::2] = code >= 1, code == 2
    called = np.repeat(code <= 2, 2, axis=1)
    geno = np.where(called, x, -1).astype(np.int8).reshape(variants, samples, 2)
    positions = np.arange(variants, dtype=np.int64) * 5 + 3
    haps = [(s, side) for s in range(samples) for side in (0, 1)]
    pop = fm.Population.from_numpy("p", geno, positions, haps, 5 * variants + 10)
    g = pop.grm()
    A = g.matrix
    values, vectors = g.eigen()
    assert values.shape == (samples,) and vectors.shape == (samples, samples) and np.all(np.diff(values) <= 0)
    assert np.abs((vectors * values) @ vectors.T - A).max() <= 1e-10 * values[0] and g.eigen()[0] is not values
    rng = np.random.default_rng(32)
    w_np, u_np = np.linalg.eigh(A)
    poly = u_np @ (np.sqrt(np.maximum(w_np, 0.0)) * rng.normal(size=samples))
    y = np.stack([(1.5 * poly if p % 2 == 0 else 0.0) + rng.normal(size=samples) + 2.0 for p in range(13)], axis=1)
    cov = rng.normal(size=(samples, 3))
    c, a = R.counts(code)

    for covariates in (None, cov):  # 13 phenotypes: one batch without covariates, two (12 + 1) with three
        scan = pop.mixed_model_scan(y, g, covariates)
        assert isinstance(scan, fm.MixedModelScan) and len(scan) == variants and scan.beta.shape == (variants, 13)
        q = 1 if covariates is None else 4
        assert scan.df == samples - q - 1 and np.array_equal(scan.positions, positions) and np.array_equal(scan.n_called, c)
        assert list(scan.covariates_kept) == ([] if covariates is None else [0, 1, 2]) and scan.covariates_dropped.size == 0
        assert np.array_equal(scan.eigenvalues, values) and scan.delta.shape == (13,) and np.allclose(scan.heritability, 1.0 / (1.0 + scan.delta))
        assert np.allclose(scan.sigma_e2, scan.delta * scan.sigma_g2) and np.isfinite(scan.log_likelihood).all() and not scan.at_boundary[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(scan.alt_frequency, a / (2.0 * c), equal_nan=True)
        for p in (0, 1, 12):  # the dense reference at the returned delta (12: the second batch)
            ref = R.dense(code[:150], A, scan.delta[p], y[:, p], covariates)
            for name in ("beta", "se", "t"):
                close(getattr(scan, name)[:150, p], ref[name], (name, p))
        # three row chunks give the same bits; so does a second run
        fmh_opts.setenv("FMH_ASSOC_BUDGET_BYTES", str(200 * 13 * (q + 2) * 8))
        chunked = pop.mixed_model_scan(y, g, covariates)
        fmh_opts.reset()
        for name in ("beta", "se", "t", "p"):
            assert np.array_equal(getattr(chunked, name), getattr(scan, name), equal_nan=True), name
        # eigenpairs from numpy instead of the library's solver
        other = pop.mixed_model_scan(y, A, covariates, eigen=(w_np[::-1].copy(), u_np[:, ::-1].copy()))
        assert np.all(np.abs(np.log10(other.delta) - np.log10(scan.delta)) <= 1e-6)
        for name in ("beta", "se", "t"):
            close(getattr(other, name), getattr(scan, name), name)
        # a plain array computes its own eigenpairs
        own = pop.mixed_model_scan(y[:, :2], A, covariates)
        for name in ("beta", "se", "t"):
            close(getattr(own, name), getattr(scan, name)[:, :2], name)

    # the identity as relationship matrix: the fixed-effects scan
    fixed = pop.association_scan(y[:, :3], cov)
    ident = pop.mixed_model_scan(y[:, :3], np.eye(samples), cov)
    for name in ("beta", "se", "t", "p"):
        close(getattr(ident, name), getattr(fixed, name), name)
    assert ident.df == fixed.df

    # variant records: a region and a sample list
    records = []
    for i in range(variants):
        calls = [None if code[i, s] == 3 else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(samples)]
        records.append(dict(position=int(positions[i]), genotypes=calls))
    chosen = [s for s in range(samples) if s % 7 != 3]
    region = (int(positions[100]) - 1, int(positions[399]) + 1)  # rows 100 .. 399
    sub = fm.grm(records, samples=chosen)
    scan = fm.mixed_model_scan(records, y[chosen, :2], sub, cov[chosen], samples=chosen, region=region)
    assert len(scan) == 300 and np.array_equal(scan.positions, positions[100:400]) and np.array_equal(scan.n_called, R.counts(code[100:400][:, chosen])[0])
    for p in (0, 1):
        ref = R.dense(code[100:250][:, chosen], sub.matrix, scan.delta[p], y[chosen, p], cov[chosen])
        for name in ("beta", "se", "t"):
            close(getattr(scan, name)[:150, p], ref[name], (name, p, "records"))
    with pytest.raises(ValueError, match="other samples"):
        fm.mixed_model_scan(records, y[chosen, :2], g, samples=chosen)
