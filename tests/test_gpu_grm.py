"""The genomic relationship matrix on the device (fmh_grm, fmh_grm_eigen) against tests/grm_ref.py, the numpy oracle written from the
definition.  Cohorts and uploads are test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2.

Integers (c, a, usable, N) are array_equal.  S is compared entry by entry with a DERIVED tolerance: any summation order of m f64 products
is within (m + 2) 2^-53 sum_k |z_ik| |z_jk| of the exact value (tests/test_gpu_pca.py derives it for the same pipe), numpy's own sum has
the same bound, so twice that separates the two; m = the usable rows plus the split count (the slab reduce adds one term per split).  The
matrix A is bitwise fmh_grm_finish of the device's S.

Shapes are the smallest at which each part can go wrong: samples 1, 2, 63 .. 65, 127 .. 129, 257 (wave tile, workgroup tile, a second tile
row, the idle lower-left wave block of a diagonal tile) in matrices of n and n + 3 samples and under sample lists; 1, 63 .. 65, 255 .. 257 and
1 030 rows (word and stage edges, several stages), both as the kept rows and as the exact number of USABLE rows - the Gram runs over those;
FMH_GRM_SPLITS 1, 2, 3 at 1 030 usable rows (the last split is shorter) and the library's own split count above 4 096.
Preconditions are asserted on the oracle alone, before the device is called, for every cohort of 255 rows and more, so that a transposed,
class-confused or mask-blind kernel cannot pass."""

import ctypes as C

import numpy as np
import pytest

from tests import grm_ref as R
from tests import pca_ref
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 63, 64, 65, 127, 128, 129, 257]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1030]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def oracle(x, called, method="standardized", samples=None, keep=None):
    code = R.codes(x, called, samples, keep)
    S, absprod, Z, usable, z, scale, m = R.products(code, method)
    c, a = R.counts(code)
    return dict(code=code, S=S, absprod=absprod, Z=Z, usable=usable, scale=scale, m=m, c=c, a=a, N=R.pair_sites(code, usable), method=method)


def preconditions(kind, ref):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 255 rows, two samples or more)."""
    code, n = ref["code"], ref["code"].shape[1]
    if n < 2:
        return
    assert not ref["usable"].all() and ref["usable"].any(), "some row is unusable, some usable"
    used = code[ref["usable"]]
    classes = (0, 1, 2, 3) if KINDS[kind][1] else (0, 1, 2)
    for cls in classes:
        assert (used == cls).any(), f"a genotype of class {cls} occurs on a usable row"
    S, bound = ref["S"], R.bound(ref["absprod"], ref["m"])
    assert np.abs(S - np.eye(n) * S[0, 0]).max() > 1000 * bound.max(), "S is not a multiple of the identity"
    swapped = R.products(code, ref["method"], swap_hom=True)[0]
    assert (np.abs(swapped - S) > 1000 * bound).any(), "hom-ref and hom-alt confused would show"
    # (two samples: a usable row with one of them missing has c = 1, a = 1, p = 0.5 and z(het) = 0 - the misreading cannot show)
    if (used == 3).any() and n >= 3:
        as_het = R.products(code, ref["method"], missing_as_het=True)[0]
        assert (np.abs(as_het - S) > 1000 * bound).any(), "a missing call read as het would show"


def check(dev, dm, x, called, what, method="standardized", samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, stream=None, ref=None,
          splits=1, pairs=True):
    """One device call (twice) against the oracle; `splits` = the split count, or an upper bound of it.  Returns the device's result."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    if ref is None:
        ref = oracle(x[row_begin : row_begin + rows], None if called is None else called[row_begin : row_begin + rows], method, sel, keep)
    params = dev.grm_params(method, "pairs" if pairs and method == "standardized" else "sites")
    kw = dict(params=params, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, keep=keep, pairs=pairs, stream=stream)
    got = dev.grm(dm, **kw)
    again = dev.grm(dm, **kw)
    # 1. integers
    assert got.kept_rows == ref["code"].shape[0], what
    assert np.array_equal(got.called, ref["c"]) and np.array_equal(got.allele_count, ref["a"]) and np.array_equal(got.usable, ref["usable"]), what
    assert got.n_usable == ref["m"] and np.float64(got.scale).view(np.uint64) == np.float64(ref["scale"]).view(np.uint64), what
    if pairs:
        assert got.pair_sites.dtype == np.uint64 and np.array_equal(got.pair_sites, ref["N"]), what
    # 2. S entry by entry
    err, bound = np.abs(got.products - ref["S"]), R.bound(ref["absprod"], ref["m"] + splits)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print(f"grm {what}: m {ref['m']}, max err {float(err.max()):.3e}, worst err/bound {worst:.3e}")
    assert np.all(err <= bound), (what, worst)
    # 3. symmetry and repeatability
    assert np.array_equal(got.products, got.products.T), what
    assert np.array_equal(got.products.view(np.uint64), again.products.view(np.uint64)), what
    # 4. A: bitwise the library's finish of the device's S, which is bitwise the oracle's
    A = dev.grm_finish(got.products, got.pair_sites if params.denominator == 1 else None, got.n_usable, got.scale, params)
    with np.errstate(divide="ignore", invalid="ignore"):
        A_ref = R.matrix(got.products, ref["N"], method, dev.GRM_DENOMINATORS[params.denominator], ref["m"], ref["scale"])
    assert np.array_equal(np.isnan(A), np.isnan(A_ref)) and np.array_equal(A.view(np.uint64)[~np.isnan(A)], A_ref.view(np.uint64)[~np.isnan(A_ref)]), what
    return got


# ---- samples: wave and workgroup tile edges, both upload forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_sample_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    rows = 257
    for n in SAMPLES:
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=5)
            ref = oracle(x, called, samples=None if extra == 0 else list(range(n)))
            preconditions(kind, ref)
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                check(dev, dm, x, called, (kind, planes, n, extra), n_samples=n, ref=ref, pairs=n in (2, 65, 129))
            finally:
                dm.close()


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists(dev, kind, method):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7)
    for total in (3, 68, 260):  # a partial byte; 65 + 3 samples cross a 128-column vector; a list longer than one group of 256 samples
        x, called = cohort(300, 2 * total, max_allele, missing, seed=26)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            gaps = np.flatnonzero(rng.random(total) < 0.6)
            if gaps.size == 0:
                gaps = np.array([total - 1])
            lists = {"none": None, "all": np.arange(total), "gaps": gaps, "last-two": np.arange(max(total - 2, 0), total)}
            for name, samples in lists.items():
                ref = oracle(x, called, method, samples)
                preconditions(kind, ref)
                check(dev, dm, x, called, (kind, method, total, name), method, samples=samples, ref=ref, pairs=name == "gaps")
            if total == 68:
                check(dev, dm, x, called, (kind, method, total, "first 65"), method, n_samples=65)
        finally:
            dm.close()


# ---- rows and keep masks: word and stage edges ------------------------------------------------------------------------------------------------
def keep_masks(rows, seed):
    rng = np.random.default_rng(rows + seed)
    first, last = np.zeros(rows, dtype=bool), np.zeros(rows, dtype=bool)
    first[0] = True
    last[-1] = True
    masks = {"null": None, "ones": np.ones(rows, dtype=bool), "half": rng.random(rows) < 0.5, "first": first, "last": last,
             "none": np.zeros(rows, dtype=bool)}
    if rows > 256:
        exact = np.zeros(rows, dtype=bool)
        exact[rng.choice(rows, size=256, replace=False)] = True
        masks["exactly-256"] = exact
    return masks


@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rows_and_keep_masks(dev, fmh_opts, kind, row_hi):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    n = 6
    for rows in ROWS:
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=8)
        if rows >= 255:
            preconditions(kind, oracle(x, called))
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            for name, keep in keep_masks(rows, 3).items():
                got = check(dev, dm, x, called, (kind, row_hi, rows, name), keep=keep)
                if name == "none":
                    assert got.kept_rows == 0 and got.n_usable == 0 and not got.products.any() and not got.pair_sites.any()
            if rows > 2:  # a row range inside the matrix, with and without a mask over it
                r0, rc = rows // 3, rows - rows // 3 - 1
                check(dev, dm, x, called, (kind, row_hi, rows, "range"), row_begin=r0, row_count=rc)
                check(dev, dm, x, called, (kind, row_hi, rows, "range+mask"), row_begin=r0, row_count=rc, keep=keep_masks(rc, 4)["half"])
        finally:
            dm.close()


def exactly_usable(x, called, k, samples=None):
    """A keep mask with exactly k usable rows (the first k of the cohort) and every third of the rows before the last of them that are not."""
    ref = oracle(x, called, samples=samples)
    usable_rows = np.flatnonzero(ref["usable"])
    assert usable_rows.size >= k, "the cohort holds enough usable rows"
    keep = np.zeros(x.shape[0], dtype=bool)
    keep[usable_rows[:k]] = True
    others = np.flatnonzero(~ref["usable"])
    keep[others[(others < usable_rows[k - 1]) & (np.arange(others.size) % 3 == 0)]] = True
    return keep


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_usable_rows_at_word_and_stage_edges(dev, kind):
    max_allele, missing = KINDS[kind]
    n = 70
    x, called = cohort(1500, 2 * n, max_allele, missing, seed=13)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for k in ROWS:
            keep = exactly_usable(x, called, k)
            ref = oracle(x, called, keep=keep)
            assert ref["m"] == k and (ref["code"].shape[0] > k or k == 1)
            if k >= 255:
                preconditions(kind, ref)
            check(dev, dm, x, called, (kind, "usable", k), keep=keep, ref=ref, pairs=k in (64, 257))
    finally:
        dm.close()


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("splits", ["1", "2", "3", None], ids=["splits=1", "splits=2", "splits=3", "splits=default"])
def test_split_k(dev, fmh_opts, splits, method):
    """1 030 usable rows = 17 words = 5 stages: two splits take 12 and 8 words, three 8, 8 and 4.  The library's own count needs more than
    4 096 rows: a split keeps at least 8 stages, so 4 160 usable rows and more make two."""
    n = 130  # three tiles: the diagonal ones and one off the diagonal
    if splits is None:
        x, called = cohort(6000, 2 * n, 1, True, seed=14)
        ref = oracle(x, called, method)
        stages = (ref["m"] + 255) // 256
        assert ref["m"] > 4096 and stages // 8 >= 2, "enough usable rows for the library to split"
        keep, bound_splits = None, stages // 8  # the count is min(what fills the device, stages / 8): at most this
    else:
        fmh_opts.setenv("FMH_GRM_SPLITS", splits)
        x, called = cohort(1500, 2 * n, 1, True, seed=14)
        keep = exactly_usable(x, called, 1030)
        ref = oracle(x, called, method, keep=keep)
        assert ref["m"] == 1030
        bound_splits = int(splits)
    preconditions("missing", ref)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    try:
        check(dev, dm, x, called, ("splits", splits, method), method, keep=keep, ref=ref, splits=bound_splits, pairs=False)
    finally:
        dm.close()


# ---- against the haplotype Gram: the route this kernel replaces -------------------------------------------------------------------------------
def test_equals_the_folded_haplotype_gram(dev):
    """Complete biallelic data: z(g) = the sum over the sample's two haplotypes of (bit - p) / sd_g, sd_g = sqrt(2 p (1 - p)), so S is the
    2 x 2 fold of fmh_pca_gram's Gram with set = (1 - p) / sd_g, clear = -p / sd_g, times its divisor n_hap - 1.  Both device sums are within
    (m + 2) eps |.||.|^T of their exact values; the fold adds the product with n_hap - 1 and three additions (4 more terms)."""
    n, rows = 130, 700
    x, _ = cohort(rows, 2 * n, 1, False, seed=15)
    ref = oracle(x, None)
    preconditions("complete", ref)
    keep = ref["usable"].copy()
    kept = np.flatnonzero(keep)
    ref = oracle(x, None, keep=keep)
    m = ref["m"]
    assert m == kept.size and m > 256
    p = ref["a"].astype(np.float64) / (2.0 * ref["c"].astype(np.float64))
    sd = np.sqrt(2.0 * p * (1.0 - p))
    hi, lo = (1.0 - p) / sd, (0.0 - p) / sd
    dm = upload(dev, x, None, 1, True, ploidy=2)
    try:
        got = check(dev, dm, x, None, "fold", keep=keep, ref=ref)
        G = dev.pca_gram(dm, kept.astype(np.uint64), hi, lo) * float(2 * n - 1)
    finally:
        dm.close()
    fold = G[0::2, 0::2] + G[0::2, 1::2] + G[1::2, 0::2] + G[1::2, 1::2]
    zh = np.abs(np.where(x[kept].T == 1, hi[None, :], lo[None, :]))
    ah = zh @ zh.T
    fold_abs = ah[0::2, 0::2] + ah[0::2, 1::2] + ah[1::2, 0::2] + ah[1::2, 1::2]
    bound = R.bound(ref["absprod"], m + 1) + 2.0 * (m + 6) * R.EPS * fold_abs
    err = np.abs(got.products - fold)
    print(f"fold: worst err/bound {float((err / bound).max()):.3e}")
    assert np.all(err <= bound)


# ---- calling conventions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_adds_accumulates_and_runs_on_a_stream(dev, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n = 70
    xa, ca = cohort(300, 2 * n, max_allele, missing, seed=10)
    xb, cb = cohort(513, 2 * n, max_allele, missing, seed=11)
    ma, mb = upload(dev, xa, ca, max_allele, True, ploidy=2), upload(dev, xb, cb, max_allele, False, ploidy=2)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        sa = check(dev, ma, xa, ca, (kind, "a, on a stream"), stream=handle)
        sb = check(dev, mb, xb, cb, (kind, "b"))
        # buffers that are not zero beforehand: the call adds (one f64 addition per entry, so numpy's sum has the same bits)
        rng = np.random.default_rng(3)
        fill = rng.normal(size=(n, n))
        fill = fill + fill.T
        fill_n = np.arange(n * n, dtype=np.uint64) * np.uint64(1 << 33) + np.uint64(5)
        bufs = dev.GrmBuffers(ma.device, n, pairs=True, fill=fill.reshape(-1), fill_pairs=fill_n)
        got = dev.grm(ma, pairs=True, into=bufs, stream=handle)
        assert np.array_equal(got.products.view(np.uint64), (fill + sa.products).view(np.uint64))
        assert np.array_equal(got.pair_sites, fill_n.reshape(n, n) + sa.pair_sites)
        # two matrices of the same samples accumulate
        bufs = dev.GrmBuffers(ma.device, n, pairs=True)
        dev.grm(ma, pairs=True, into=bufs, stream=handle)
        got = dev.grm(mb, pairs=True, into=bufs, stream=handle)
        assert np.array_equal(got.products.view(np.uint64), (sa.products + sb.products).view(np.uint64))
        assert np.array_equal(got.pair_sites, sa.pair_sites + sb.pair_sites)
        assert got.n_usable == sb.n_usable and got.scale == sb.scale  # this call's: the caller adds them up
        stream.synchronize()
    finally:
        ma.close()
        mb.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_launch_error(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    bufs = dev.GrmBuffers(dm.device, 8, pairs=True)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    full = _abi.GrmOut(bufs.products.ptr, bufs.pair_sites.ptr, None, None, None, None, None)
    std, cen_pairs, std_pairs = _abi.GrmParams(0, 0), _abi.GrmParams(1, 1), _abi.GrmParams(0, 1)

    def call(m=dm, samples=None, n=8, r0=0, rc=40, k=None, o=full, P=std):
        return lib.fmh_grm(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if k is None else p(k),
                           None if P is None else C.byref(P), None if o is None else C.byref(o), None, None)

    try:
        invalid = [call(m=None), call(P=None), call(o=None), call(o=_abi.GrmOut(None, bufs.pair_sites.ptr, None, None, None, None, None)),
                   call(P=_abi.GrmParams(2, 0)), call(P=_abi.GrmParams(0, 2)), call(P=cen_pairs),
                   call(P=std_pairs, o=_abi.GrmOut(bufs.products.ptr, None, None, None, None, None, None)), call(n=0), call(n=9),
                   call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2), call(samples=u32(4, 2), n=2), call(r0=41, rc=0), call(r0=1, rc=40),
                   call(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=haploid, n=0) == _abi.FMH_ERR_INVALID            # the order: n_samples before the ploidy,
        assert call(m=haploid, n=99) == _abi.FMH_ERR_UNSUPPORTED       # the ploidy before the samples,
        assert call(m=unpacked, r0=41, rc=0) == _abi.FMH_ERR_INVALID   # the rows before the packed image
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_PCA_BUDGET_BYTES", "1000")
        assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_PCA_BUDGET_BYTES" in lib.fmh_last_error()
        fmh_opts.reset()
        # nothing was added by a refused call, no launch error is left behind, and a kept list of nothing adds nothing
        assert call(k=np.zeros(40, dtype=np.uint8)) == 0
        assert not bufs.products.to_numpy(np.float64, 64).any() and not bufs.pair_sites.to_numpy(np.uint64, 64).any()
        check(dev, dm, x, called, "after the refusals")
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


def test_no_usable_row_adds_nothing(dev):
    x = np.zeros((70, 12), dtype=np.uint8)
    x[::2] = 1  # every row monomorphic
    dm = upload(dev, x, None, 1, True, ploidy=2)
    try:
        fill = np.full(36, 2.5)
        bufs = dev.GrmBuffers(dm.device, 6, pairs=True, fill=fill)
        got = dev.grm(dm, pairs=True, into=bufs)
        assert got.kept_rows == 70 and got.n_usable == 0 and got.scale == 0.0 and not got.usable.any()
        assert np.array_equal(got.products.reshape(-1), fill) and not got.pair_sites.any()
    finally:
        dm.close()


# ---- eigenpairs -----------------------------------------------------------------------------------------------------------------------------------
def structured_cohort(variants, samples, populations, seed):
    """pca_ref.pybench_cohort (populations drifted apart) folded to alleles [variants][2 * samples]: populations - 1 gapped eigenvalues."""
    g = pca_ref.pybench_cohort(variants, samples, seed, scale=0.15, populations=populations)
    return np.ascontiguousarray(g.reshape(variants, 2 * samples).astype(np.uint8))


def cpu_pair(x, k):
    """(eigenvalues [k], eigenvectors [n][k], d0, A) - and the check that this CPU pair is conclusive, before any device result is looked at."""
    ref = oracle(x, None)
    A = ref["S"] / float(ref["m"])
    w, a, b, d0, all_w = R.eigen_pair(A, ref["Z"], ref["m"], k)
    assert 32 * d0 <= 1e-8 * np.abs(a).max(), ("CPU pair inconclusive", d0)
    gaps = (all_w[:k] - all_w[1 : k + 1]) / all_w[0]
    assert gaps.min() >= 1e-2, ("the requested eigenvalues are not gapped", gaps)
    return w, a, d0, A


@pytest.mark.parametrize("variants,samples,populations", [(3000, 60, 3), (6000, 131, 5)])
def test_eigenpairs(dev, fmh_opts, variants, samples, populations):
    x = structured_cohort(variants, samples, populations, seed=variants + samples)
    k = populations - 1
    w, a, d0, A = cpu_pair(x, k)
    results = {}
    for solver in ("rocsolver", "host"):
        fmh_opts.setenv("FMH_PCA_EIGEN", solver)
        values, vectors = dev.grm_eigen(0, A, k)
        results[solver] = vectors
        err = float(np.abs(vectors - a).max())
        print(f"eigen {solver} n={samples}: vector err {err:.3e}, 32*d0 {32 * d0:.3e}")
        assert err <= 32 * d0, (solver, err, d0)
        assert np.all(np.abs(values - w) <= 32 * d0 * np.abs(w[0])), (solver, values, w)
        assert np.all(np.abs(np.linalg.norm(vectors, axis=0) - 1.0) <= 1e-12)
        assert np.all(vectors[np.argmax(np.abs(vectors), axis=0), np.arange(k)] > 0), "the largest component is positive"
    assert np.abs(results["rocsolver"] - results["host"]).max() <= 64 * d0


# ---- through `import ferromic` ------------------------------------------------------------------------------------------------------------------------
def test_python_surface_end_to_end(fm):
    from tests import assoc_ref

    variants, samples, populations = 2000, 48, 5
    x = structured_cohort(variants, samples, populations, seed=77)
    x[5::10] = x[4::10]  # a tenth of the rows repeat their neighbour: ld_prune has something to drop
    rng = np.random.default_rng(5)
    called = rng.random((variants, samples)) >= 0.01
    called = np.repeat(called, 2, axis=1)
    geno = np.where(called, x, -1).astype(np.int8).reshape(variants, samples, 2)
    positions = np.arange(variants, dtype=np.int64) * 5 + 3
    haps = [(s, side) for s in range(samples) for side in (0, 1)]
    pop = fm.Population.from_numpy("p", geno, positions, haps, 5 * variants + 10)
    keep = pop.ld_prune(20, 0.8)
    assert keep.dtype == bool and 100 < keep.sum() < variants

    for method, denominator in (("standardized", "sites"), ("standardized", "pairs"), ("centered", "sites")):
        ref = oracle(x, called, method, keep=keep)
        g = pop.grm(sites=keep, method=method, denominator=denominator)
        assert isinstance(g, fm.GeneticRelationship)
        assert np.array_equal(g.samples, np.arange(samples)) and np.array_equal(g.sites, np.flatnonzero(keep))
        assert np.array_equal(g.usable, ref["usable"]) and g.n_usable == ref["m"] and g.usable.dtype == bool
        assert np.array_equal(g.called, ref["c"]) and np.array_equal(g.allele_count, ref["a"])
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(g.frequency, R.values(ref["c"], ref["a"], method)[1], equal_nan=True)
        assert np.float64(g.scale).view(np.uint64) == np.float64(ref["scale"]).view(np.uint64)
        assert np.all(np.abs(g.products - ref["S"]) <= R.bound(ref["absprod"], ref["m"] + 1))
        if denominator == "pairs":
            assert np.array_equal(g.pair_sites, ref["N"])
        else:
            assert g.pair_sites is None
        A = R.matrix(g.products, ref["N"], method, denominator, ref["m"], ref["scale"])
        assert np.array_equal(g.matrix.view(np.uint64), A.view(np.uint64))
        assert np.array_equal(g.inbreeding(), np.diag(A) - 1.0)

    # the eigenvectors as covariates of the association scan
    ref = oracle(x, called, keep=keep)
    A = ref["S"] / float(ref["m"])
    w, a, b, d0, all_w = R.eigen_pair(A, ref["Z"], ref["m"], 4)
    assert 32 * d0 <= 1e-8 * np.abs(a).max() and ((all_w[:4] - all_w[1:5]) / all_w[0]).min() >= 1e-2
    g = pop.grm(sites=keep)
    pcs = g.pca(4)
    assert isinstance(pcs, fm.GenotypePCA) and pcs.eigenvectors.shape == (samples, 4) and pcs.eigenvectors.dtype == np.float64
    assert np.array_equal(pcs.samples, np.arange(samples))
    # the device's A is within bound / m of the oracle's entry by entry, so within samples * that in the 2-norm; an eigenvector moves by at most
    # the 2-norm over its eigenvalue's gap
    gap = float((all_w[:4] - all_w[1:5]).min())
    moved = samples * float(R.bound(ref["absprod"], ref["m"] + 1).max()) / float(ref["m"]) / gap
    assert np.abs(pcs.eigenvectors - a).max() <= 32 * d0 + moved
    assert np.all(np.abs(pcs.eigenvalues - w) <= 1e-9 * w[0])
    assert np.allclose(pcs.explained, pcs.eigenvalues / np.trace(g.matrix), rtol=1e-14, atol=0)
    assert g.pca(1000).eigenvectors.shape == (samples, samples)
    y = rng.normal(size=(samples, 2)) + 3.0
    y[:, 0] += 0.8 * a[:, 0] * np.sqrt(samples)
    scan = pop.association_scan(y, pcs.eigenvectors)
    # the scan is its own oracle's, bit for bit, on the covariates it was given ...
    prep = assoc_ref.prepare(y, pcs.eigenvectors)
    S, Cs = assoc_ref.sums(x, called, prep["values"], None)
    trk = assoc_ref.tracks(x, called, None)
    same = assoc_ref.stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], samples, prep["n_basis"])
    for name in ("beta", "se", "t", "p"):
        assert assoc_ref.same_f64(getattr(scan, name), same[name]), name
    assert scan.covariates_dropped.size == 0
    # ... and equals the scan fed the oracle's vectors within what the covariates differ by: they agree to 1e-8 of their largest entry (asserted
    # above) and the scan itself quantises a covariate column to 2^-30 of its largest entry; its statistics are smooth in the covariates, so
    # 1e-6 of the largest statistic of a phenotype is three orders above both
    other = pop.association_scan(y, a)
    for name in ("beta", "t"):
        got, want = getattr(scan, name), getattr(other, name)
        ok = np.isfinite(want)
        assert np.array_equal(ok, np.isfinite(got))
        assert np.all(np.abs(got - want)[ok] <= 1e-6 * np.abs(want[ok]).max()), name

    # a NaN in the matrix: a pair without a jointly called usable site
    holes = called.copy()
    holes[:, 0:2] = np.arange(variants)[:, None] % 2 == 0
    holes[:, 2:4] = np.arange(variants)[:, None] % 2 == 1
    geno = np.where(holes, x, -1).astype(np.int8).reshape(variants, samples, 2)
    g = fm.Population.from_numpy("p", geno, positions, haps, 5 * variants + 10).grm(denominator="pairs")
    assert np.isnan(g.matrix[0, 1]) and g.pair_sites[0, 1] == 0
    with pytest.raises(ValueError, match='denominator="pairs"'):
        g.pca(2)
    with pytest.raises(ValueError):
        pop.grm(sites=np.ones(variants - 1, dtype=bool))


def test_grm_of_variant_records(fm):
    x, called = cohort(60, 24, 1, True, seed=24)
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(12)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    samples = [1, 2, 5, 10, 11]
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    for kw, ref in ((dict(), oracle(x, eff_called)), (dict(samples=samples), oracle(x, eff_called, samples=samples)),
                    (dict(region=region, method="centered"), oracle(x[6:52], eff_called[6:52], "centered"))):
        g = fm.grm(variants, **kw)
        assert np.array_equal(g.usable, ref["usable"]) and np.array_equal(g.called, ref["c"]) and np.array_equal(g.allele_count, ref["a"])
        assert np.all(np.abs(g.products - ref["S"]) <= R.bound(ref["absprod"], ref["m"] + 1))
        assert np.array_equal(g.samples, np.arange(12) if "samples" not in kw else np.asarray(samples))
