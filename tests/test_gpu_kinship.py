"""Relatedness on the device (fmh_kinship_counts) against tests/kinship_ref.py, the numpy oracle written from the definition.  Every
comparison of tables is array_equal on u64; kinship and IBS distance are compared bitwise with the oracle's.  Cohorts and uploads are
test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2.

Shapes are the smallest at which each part can go wrong:
  * samples 1, 2, 3, 64, 127 .. 129, 255 .. 257, 300: the all-ones row and the V block land on, before and after a 256-row tile edge of the
    stacked operand in both routes (complete: ones at row n; general: V from row n, ones at row 2n); matrices of n and of n + 3 samples;
  * rows around the 256-site FP4 K block and the 128-site int8 one, 1 300 for several K blocks;
  * 700 / 1 300 / 513 rows with FMH_PD_PLANES_BYTES=1 for three and more row slabs; 9 000 to 20 000 rows for several K slices of an
    item (an item takes at least 4 096 K bytes = 8 192 FP4 sites before it is cut).
Preconditions are asserted on the oracle alone, before the device is called, for every cohort of 255 rows and more, so that a transposed,
symmetrised or mask-blind kernel cannot pass."""

import ctypes as C

import numpy as np
import pytest

from tests import kinship_ref
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 3, 64, 127, 128, 129, 255, 256, 257, 300]
ROWS = [1, 2, 127, 128, 129, 255, 256, 257, 511, 513, 1300]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def preconditions(kind, x, called, samples=None):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 255 rows).  Returns the oracle's tables."""
    max_allele, missing = KINDS[kind]
    both, het_het, ibs0, het_hom = kinship_ref.tables(x, called, samples)
    n = both.shape[0]
    if n >= 2:
        off = ~np.eye(n, dtype=bool)
        assert (both[off] > 0).all(), "every pair shares a called row"
        assert (ibs0 > 0).any(), "some pair is opposite homozygous somewhere"
        assert (het_hom != het_hom.T).any(), "het_hom is not symmetric"
    if missing:
        assert (both < x.shape[0]).any(), "a missing call lowers some count"
    if max_allele > 1:
        high = x > 1
        if called is not None:
            high &= called
        cols = slice(None) if samples is None else np.concatenate([[2 * s, 2 * s + 1] for s in samples])
        assert high[:, cols].any(), "an upper allele plane un-calls some genotype"
    return both, het_het, ibs0, het_hom


def check(dev, dm, x, called, what, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, stream=None, ref=None):
    """One device call against the oracle (`ref`: its tables for exactly these arguments, when the caller has them); returns the device's."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    if ref is None:
        ref = kinship_ref.tables(x[row_begin : row_begin + rows], None if called is None else called[row_begin : row_begin + rows], sel, keep)
    got = dev.kinship_counts(dm, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, keep=keep, stream=stream)
    for name, r in zip(dev.KINSHIP_TABLES, ref):
        g = getattr(got, name)
        assert g.dtype == np.uint64 and g.shape == r.shape, (what, name)
        assert np.array_equal(g, r), (what, name, np.argwhere(g != r)[:4].tolist())
    assert got.kept_rows == (rows if keep is None else int(np.count_nonzero(keep))), what
    phi, dist = dev.kinship_stats(got.both, got.het_het, got.ibs0, got.het_hom)
    ref_phi, ref_dist = kinship_ref.stats(*ref)
    assert np.array_equal(phi.view(np.uint64)[np.isfinite(ref_phi)], ref_phi.view(np.uint64)[np.isfinite(ref_phi)]), what
    assert np.array_equal(np.isnan(phi), np.isnan(ref_phi)) and np.array_equal(dist, ref_dist, equal_nan=True), what
    return got


# ---- samples: tile edges of the stacked operand, in both routes, both upload forms -------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_sample_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    rows = 257
    for n in SAMPLES:
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=5)
            ref = preconditions(kind, x, called, None if extra == 0 else list(range(n)))
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                check(dev, dm, x, called, (kind, planes, n, extra), n_samples=n, ref=ref)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists(dev, kind):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7)
    for total in (3, 68, 260):  # a partial byte; 65 + 3 samples cross a 128-column vector; a list longer than one sample block
        x, called = cohort(300, 2 * total, max_allele, missing, seed=26)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            gaps = np.flatnonzero(rng.random(total) < 0.6)
            if gaps.size == 0:
                gaps = np.array([total - 1])
            lists = {"none": None, "all": np.arange(total), "gaps": gaps, "last-two": np.arange(max(total - 2, 0), total)}
            for name, samples in lists.items():
                ref = preconditions(kind, x, called, samples)
                check(dev, dm, x, called, (kind, total, name), samples=samples, ref=ref)
            if total == 68:
                check(dev, dm, x, called, (kind, total, "first 65"), n_samples=65)
        finally:
            dm.close()


# ---- rows and keep masks: around the K block of both operand formats --------------------------------------------------------------------
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


@pytest.mark.parametrize("int8", [False, True], ids=["fp4", "int8"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rows_and_keep_masks(dev, fmh_opts, kind, int8):
    max_allele, missing = KINDS[kind]
    if int8:
        fmh_opts.setenv("FMH_PD_INT8", "1")
    n = 6
    for rows in ROWS:
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=8)
        if rows >= 255:
            preconditions(kind, x, called)
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            for name, keep in keep_masks(rows, 3).items():
                got = check(dev, dm, x, called, (kind, int8, rows, name), keep=keep)
                if name == "none":
                    assert got.kept_rows == 0 and not got.both.any()
            if rows > 2:  # a row range inside the matrix, with and without a mask over it
                r0, rc = rows // 3, rows - rows // 3 - 1
                check(dev, dm, x, called, (kind, int8, rows, "range"), row_begin=r0, row_count=rc)
                check(dev, dm, x, called, (kind, int8, rows, "range+mask"), row_begin=r0, row_count=rc, keep=keep_masks(rc, 4)["half"])
        finally:
            dm.close()


# ---- routes of the shared Gram launcher ----------------------------------------------------------------------------------------------------
ROUTES = {
    "int8": ({"FMH_PD_INT8": "1"}, [(3, 700), (129, 1300), (257, 513)]),
    "unphased": ({"FMH_PD_PHASED": "0"}, [(3, 700), (129, 1300), (257, 513)]),
    "unphased-int8": ({"FMH_PD_PHASED": "0", "FMH_PD_INT8": "1"}, [(3, 700), (129, 1300), (257, 513)]),
    "atomics": ({"FMH_PD_SLABS": "0"}, [(3, 700), (129, 1300), (257, 513)]),
    "row-slabs": ({"FMH_PD_PLANES_BYTES": "1"}, [(3, 700), (129, 1300), (257, 513)]),       # one K block per slab: 3, 6 and 3 slabs (FP4)
    "row-slabs-int8": ({"FMH_PD_PLANES_BYTES": "1", "FMH_PD_INT8": "1"}, [(3, 700), (129, 1300), (257, 513)]),
    "k-slices": ({"FMH_PD_KCHUNK": "128"}, [(3, 20000), (70, 12000), (129, 9000)]),          # 10 000 / 6 000 / 4 500 K bytes: 3 / 2 / 2 slices
    "k-slices-atomics": ({"FMH_PD_KCHUNK": "128", "FMH_PD_SLABS": "0"}, [(3, 20000), (70, 12000), (129, 9000)]),
}


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])  # the complete route and the general one
@pytest.mark.parametrize("route", list(ROUTES))
def test_gram_routes(dev, fmh_opts, route, kind):
    max_allele, missing = KINDS[kind]
    options, shapes = ROUTES[route]
    for n, rows in shapes:
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=9)
        ref = preconditions(kind, x, called)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            check(dev, dm, x, called, (route, kind, n, rows, "default"), ref=ref)
            for key, value in options.items():
                fmh_opts.setenv(key, value)
            half = np.random.default_rng(rows).random(rows) < 0.5
            check(dev, dm, x, called, (route, kind, n, rows), ref=ref)
            check(dev, dm, x, called, (route, kind, n, rows, "half"), keep=half)
            fmh_opts.reset()
        finally:
            dm.close()


# ---- calling conventions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complete", "missing", "multi7"])
def test_adds_accumulates_and_repeats_on_a_stream(dev, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n = 70
    xa, ca = cohort(300, 2 * n, max_allele, missing, seed=10)
    xb, cb = cohort(513, 2 * n, max_allele, missing, seed=11)
    preconditions(kind, xa, ca)
    preconditions(kind, xb, cb)
    ma, mb = upload(dev, xa, ca, max_allele, True, ploidy=2), upload(dev, xb, cb, max_allele, False, ploidy=2)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        # buffers that are not zero beforehand: the call adds
        fill = np.arange(n * n, dtype=np.uint64) * np.uint64(1 << 33) + np.uint64(5)
        bufs = dev.KinshipBuffers(ma.device, n, fill=fill)
        got = dev.kinship_counts(ma, into=bufs, stream=handle)
        ref_a = kinship_ref.tables(xa, ca)
        for name, r in zip(dev.KINSHIP_TABLES, ref_a):
            assert np.array_equal(getattr(got, name), r + fill.reshape(n, n)), name
        # two matrices of the same samples accumulate: the oracle on their concatenation
        bufs = dev.KinshipBuffers(ma.device, n)
        dev.kinship_counts(ma, into=bufs, stream=handle)
        got = dev.kinship_counts(mb, into=bufs, stream=handle)
        ref = kinship_ref.tables(np.concatenate([xa, xb]), None if ca is None else np.concatenate([ca, cb]))
        for name, r in zip(dev.KINSHIP_TABLES, ref):
            assert np.array_equal(getattr(got, name), r), name
        # the same input twice: the same bits
        again = dev.kinship_counts(mb, stream=handle)
        once = dev.kinship_counts(mb)
        for name in dev.KINSHIP_TABLES:
            assert np.array_equal(getattr(again, name), getattr(once, name)), name
        stream.synchronize()
    finally:
        ma.close()
        mb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_launch_error(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    bufs = dev.KinshipBuffers(dm.device, 8)
    out = C.byref(bufs.out)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    keep = np.ones(40, dtype=np.uint8)

    def call(m=dm, samples=None, n=8, r0=0, rc=40, k=None, o=out):
        return lib.fmh_kinship_counts(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if k is None else p(k), o, None,
                                      None)

    try:
        assert call() == 0
        invalid = [call(m=None), call(o=None), call(n=0), call(n=9), call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2),
                   call(samples=u32(4, 2), n=2), call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        for k in range(4):
            ptrs = [b.ptr for b in bufs.bufs]
            ptrs[k] = None
            assert call(o=C.byref(_abi.KinshipOut(*ptrs))) == _abi.FMH_ERR_INVALID
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_KIN_BUDGET_BYTES", "1000")  # 8 samples, general route: 17^2 * 8 + 64 * 8 = 2 824 bytes
        assert call() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_KIN_BUDGET_BYTES" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_KIN_BUDGET_BYTES", "2824")
        assert call() == 0
        fmh_opts.reset()
        # nothing was added by a refused call, no launch error is left behind, and a kept list of nothing adds nothing
        assert call(k=np.zeros(40, dtype=np.uint8)) == 0
        both = bufs.tables()[0]
        assert np.array_equal(both, 2 * kinship_ref.tables(x, called)[0])
        check(dev, dm, x, called, "after the refusals", keep=keep)
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- through `import ferromic` --------------------------------------------------------------------------------------------------------------
def assert_kinship(k, x, called, samples, keep, what):
    ref = kinship_ref.tables(x, called, samples, keep)
    for name, r in zip(("both", "het_het", "ibs0", "het_hom"), ref):
        g = getattr(k, name)
        assert g.dtype == np.uint64 and np.array_equal(g, r), (what, name)
    phi, dist = kinship_ref.stats(*ref)
    assert k.kinship.dtype == np.float64 and np.array_equal(k.kinship, phi, equal_nan=True), what
    assert np.array_equal(k.ibs_distance, dist, equal_nan=True), what
    assert np.array_equal(k.samples, np.arange(x.shape[1] // 2) if samples is None else np.asarray(samples)), what
    assert np.array_equal(k.sites, np.arange(x.shape[0]) if keep is None else np.flatnonzero(keep)), what
    for threshold in (0.0, 0.0884, 0.3):
        got = k.unrelated(threshold)
        assert got.dtype == bool and np.array_equal(got, kinship_ref.unrelated(phi, threshold)), (what, threshold)


def test_population_from_numpy(fm):
    """300 sites x 40 diploid samples with missing calls; the population holds both haplotypes of 22 samples and one of three more."""
    rng = np.random.default_rng(41)
    x, called = cohort(300, 80, 1, True, seed=41)
    preconditions("missing", x, called)
    geno = np.where(called, x, -1).astype(np.int8).reshape(300, 40, 2)
    whole = sorted(int(s) for s in rng.choice(40, size=22, replace=False))
    halves = [s for s in range(40) if s not in whole][:3]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(s, 1) for s in halves]
    pop = fm.Population.from_numpy("p", geno, np.arange(300, dtype=np.int64) * 7, haps, 3000)
    k = pop.kinship()
    assert isinstance(k, fm.Kinship)
    assert_kinship(k, x, called, whole, None, "Population.kinship")
    keep = pop.ld_prune(33, 0.2)
    assert 0 < keep.sum() < 300
    assert_kinship(pop.kinship(sites=keep), x, called, whole, keep, "Population.kinship(sites=ld_prune)")
    with pytest.raises(ValueError):
        pop.kinship(sites=np.ones(299, dtype=bool))
    with pytest.raises(TypeError):
        k.unrelated()  # the threshold is required: the library pins no cutoff


def test_kinship_of_variant_records(fm):
    """A sparse variant list (records with missing genotypes), a region that cuts rows off both ends, a sample list, ld_prune's sites."""
    x, called = cohort(60, 24, 1, True, seed=24)
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(12)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    assert_kinship(fm.kinship(variants), x, eff_called, None, None, "kinship")
    samples = [1, 2, 5, 10, 11]
    assert_kinship(fm.kinship(variants, samples=samples), x, eff_called, samples, None, "kinship(samples)")
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    assert_kinship(fm.kinship(variants, region=region), x[6:52], eff_called[6:52], None, None, "kinship(region)")
    haps = [(s, side) for s in range(12) for side in (0, 1)]
    keep = fm.ld_prune(variants, haps, 9, 0.3, region=region)
    assert keep.shape == (46,) and 0 < keep.sum() < 46
    assert_kinship(fm.kinship(variants, samples=samples, sites=keep, region=region), x[6:52], eff_called[6:52], samples, keep, "kinship(all arguments)")
    for bad in ([2, 1], [0, 0], [12], [-1]):
        with pytest.raises(ValueError):
            fm.kinship(variants, samples=bad)
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(12)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.kinship(haploid)
