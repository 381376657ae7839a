"""The admixture model's device step (fmh_admix_create, fmh_admix_step) and its Python surface against tests/admix_ref.py, the oracle written
from the definition in np.longdouble and rounded once.  Cohorts and uploads are test_gpu_sfs.py's (multi-allelic rows, missing calls, random
bits under the uncalled entries of every allele plane), with ploidy 2.

Tolerance, derived.  u = 2^-53.  Every sum of the step has only non-negative terms, so a sum of N such terms in ANY order (the kernel's: four
at a time inside an MFMA, tiles, waves and items in their fixed order) is within (N + 2) u of itself RELATIVELY.  Following the chain:
h0, h1 are K products summed: (K + 2) u.  u = g / h0 and v = (2 - g) / h1 add one division (and G = fl(1 - F) one rounding): (K + 4) u.
A, B sum n products u q: (n + K + 8) u.  f' = f A / (f A + g B): numerator and denominator carry (n + K + 8) u plus two products and a sum,
the quotient at most twice that: f' is within 2 (n + K + 16) u f'.  E sums 2 m products: (2 m + K + 8) u.  q0 = q E / (2 m_i) and the
renormalisation by a sum of K terms: q' is within 2 (2 m + 2 K + 24) u q'.  Clamps are non-expansive.  For l, with Gamma the number of called
genotypes of usable rows, each term g log h0 + (2 - g) log h1 carries 2 (K + 2) u from h absolutely (d log h = dh / h), a few ulp of log and,
where a lane multiplies up to 16 factors before one log, 16 u more: 2 (K + 40) u per genotype leaves room; the sum of Gamma terms of one sign
adds (2 Gamma + 2) u |l|:   |l^ - l| <= 2 Gamma (K + 40) u + (2 Gamma + 2) u |l|.
The tests assert TWICE each bound, as test_gpu_lmm.py does, and print the worst error / (2 bound).  The tracks are integers: array_equal.

Shapes are the smallest at which each part can go wrong: samples 1, 2, 15 .. 17 (the sample tile), 63 .. 65, 129, 257 in matrices of n and
n + 3 samples and under sample lists; K 1 .. 5, 8, 9, 12, 13, 16 (every KS = ceil(K / 4), both sides of each step); usable rows 1, 15 .. 17
(the row tile), 63 .. 65 (a code word), 255 .. 257 (the pass of 128 rows), 1 030; row ranges that start off a tile and keep masks;
FMH_ADMIX_ITEM_ROWS small enough that 1 030 rows are several blocks, so that the slab reduce and the l partials are exercised.  Every case
runs twice (equal bits) into NaN-filled outputs.  Preconditions are asserted on the oracle alone, before the device runs, for cohorts of 255
rows and more, so that a class-confused, mask-blind, u / v-confused, G-blind or transposed kernel cannot pass."""

import ctypes as C
import threading

import numpy as np
import pytest

from tests import admix_ref as R
from tests import grm_ref
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 129, 257]
COMPONENTS = [1, 2, 3, 4, 5, 8, 9, 12, 13, 16]
USABLE = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1030]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def state(n, m, K, seed):
    rng = np.random.default_rng(seed * 1000003 + n * 7919 + m * 31 + K)
    q = rng.dirichlet(np.full(K, 0.7), size=n).clip(R.EPS, R.HI)
    return q / q.sum(axis=1, keepdims=True), rng.uniform(0.05, 0.95, size=(m, K))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def preconditions(d, q, f, ref):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 255 rows, three samples or more)."""
    n, K = q.shape
    bf, bq, _ = R.bounds(d, K, ref[2])

    def shows(**wrong):
        oq, of, _, _ = R.step(d, q, f, **wrong)
        return (np.abs(of - ref[1]) > 1000 * 2 * bf * np.abs(ref[1])).any() or (np.abs(oq - ref[0]) > 1000 * 2 * bq * np.abs(ref[0])).any()

    usable = R.tracks(d)[0]
    assert (~usable).any(), "a row that is not usable occurs"
    assert shows(swap_hom=True), "hom-ref and hom-alt swapped would show"
    if (d[usable] == 3).any():
        assert shows(missing_as_ref=True), "a missing call read as hom-ref would show"
    assert shows(swap_uv=True), "u and v exchanged would show"
    if K > 1:
        assert shows(g_is_f=True), "G replaced by F would show"
    if K == n and n > 1:
        assert shows(transpose_q=True), "Q read transposed would show"


def compare(got, ref, d, K, what):
    """A device step (q', f', l) against the oracle's within twice the bounds."""
    bf, bq, bl = R.bounds(d, K, ref[2])
    wf, wq = R.worst(got[1], ref[1], bf), R.worst(got[0], ref[0], bq)
    wl = 0.0 if got[2] is None or bl == 0.0 else abs(got[2] - ref[2]) / (2 * bl)
    print(f"admix {what}: worst err / (2 bound): f {wf:.3e}, q {wq:.3e}, l {wl:.3e}")
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), (what, "every entry is written")
    assert wf <= 1.0 and wq <= 1.0 and wl <= 1.0, (what, wf, wq, wl)


def check(dev, dm, x, called, what, K, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, stream=None, pre=False, seed=1):
    """One image and one device step (twice) against the oracle.  Returns (the step's result, the dosage table, the state)."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    d = grm_ref.codes(x[row_begin : row_begin + rows], None if called is None else called[row_begin : row_begin + rows], sel, keep)
    usable, c, a, sites, m = R.tracks(d)
    q, f = state(d.shape[1], m, K, seed)
    ref = R.step(d, q, f)
    if pre:
        preconditions(d, q, f, ref)
    with dev.AdmixImage(dm, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, keep=keep, stream=stream) as image:
        assert (image.n, image.kept_rows, image.m) == (d.shape[1], d.shape[0], m), what
        assert np.array_equal(image.usable, usable) and np.array_equal(image.called, c) and np.array_equal(image.allele_count, a), what
        assert np.array_equal(image.sample_sites, sites), what
        got = dev.admix_step(image, q, f, fill=np.nan, stream=stream)
        again = dev.admix_step(image, q, f, fill=-7.0, stream=stream)
    compare(got, ref, d, K, what)
    assert np.array_equal(bits(got[0]), bits(again[0])) and np.array_equal(bits(got[1]), bits(again[1])) and got[2] == again[2], what
    return got, d, (q, f)


def keep_usable(x, called, n, want):
    """A keep mask over the rows of x that keeps every row that is not usable and the first `want` usable ones."""
    usable = R.tracks(grm_ref.codes(x, called, np.arange(n)))[0]
    assert usable.sum() >= want, (usable.sum(), want)
    keep = ~usable
    keep[np.flatnonzero(usable)[:want]] = True
    return keep


# ---- samples: tile edges, both upload forms, every K -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_sample_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    for at, n in enumerate(SAMPLES):
        for extra in (0, 3):
            K = COMPONENTS[(at + extra) % len(COMPONENTS)]
            x, called = cohort(257, 2 * (n + extra), max_allele, missing, seed=5)
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                check(dev, dm, x, called, (kind, planes, n, extra, K), K, n_samples=n, pre=n >= 3)
                if n in (3, 16):
                    check(dev, dm, x, called, (kind, planes, n, extra, "K = n"), n, n_samples=n, pre=True)
            finally:
                dm.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists_and_every_component_count(dev, kind):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7)
    at = 0
    for total in (3, 68, 260):
        x, called = cohort(300, 2 * total, max_allele, missing, seed=26)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            gaps = np.flatnonzero(rng.random(total) < 0.6)
            if gaps.size == 0:
                gaps = np.array([total - 1])
            for name, samples in {"none": None, "all": np.arange(total), "gaps": gaps, "last-two": np.arange(max(total - 2, 0), total)}.items():
                n = total if samples is None else len(samples)
                for _ in range(2):
                    K = COMPONENTS[at % len(COMPONENTS)]
                    at += 1
                    check(dev, dm, x, called, (kind, total, name, K), K, samples=samples, pre=n >= 3)
            if total == 3:
                check(dev, dm, x, called, (kind, total, "K = n = 3"), 3, pre=True)
        finally:
            dm.close()


# ---- usable rows: tile, word and pass edges; ranges that start off a tile; keep masks -----------------------------------------------------------
@pytest.mark.parametrize("row_hi", ["0", "2"], ids=["row_hi=0", "row_hi=2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_usable_rows_ranges_and_keep_masks(dev, fmh_opts, kind, row_hi):
    max_allele, missing = KINDS[kind]
    fmh_opts.setenv("FMH_ROW_HI", row_hi)
    n = 20
    x, called = cohort(4200, 2 * n, max_allele, missing, seed=8)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for at, want in enumerate(USABLE):
            K = COMPONENTS[at % len(COMPONENTS)]
            keep = keep_usable(x, called, n, want)
            got, d, _ = check(dev, dm, x, called, (kind, row_hi, want, K), K, keep=keep, pre=want >= 255)
            assert got[1].shape == (want, K)
        check(dev, dm, x, called, (kind, row_hi, "range"), 5, row_begin=343, row_count=686)
        check(dev, dm, x, called, (kind, row_hi, "range from 5"), 3, row_begin=5, row_count=170)
        keep = np.random.default_rng(3).random(1000) < 0.5
        check(dev, dm, x, called, (kind, row_hi, "range and mask"), 9, row_begin=7, row_count=1000, keep=keep, pre=True)
    finally:
        dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_item_and_grid_sizes(dev, fmh_opts, kind):
    """1 030 usable rows as 1, 3 and 9 blocks on 1, 3 and the default number of workgroups: a workgroup takes several items, an item several
    passes, the last is short.  No option changes a bit of F'; the grid options change no bit at all; the item size moves Q' and l within
    the bounds."""
    max_allele, missing = KINDS[kind]
    n, K = 70, 13
    x, called = cohort(4200, 2 * n, max_allele, missing, seed=9)
    keep = keep_usable(x, called, n, 1030)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        first, d, (q, f) = check(dev, dm, x, called, (kind, "default"), K, keep=keep, pre=True)
        ref = R.step(d, q, f)
        with dev.AdmixImage(dm, keep=keep) as image:
            for item_rows in ("128", "300", "4096"):
                per_item = None
                for blocks, per_cu in ((None, None), ("1", None), ("3", None), (None, "1")):
                    fmh_opts.setenv("FMH_ADMIX_ITEM_ROWS", item_rows)
                    if blocks is not None:
                        fmh_opts.setenv("FMH_GRID_BLOCKS", blocks)
                    if per_cu is not None:
                        fmh_opts.setenv("FMH_GRID_PER_CU", per_cu)
                    got = dev.admix_step(image, q, f, fill=np.nan)
                    fmh_opts.reset()
                    assert np.array_equal(bits(got[1]), bits(first[1])), (item_rows, blocks, per_cu, "no bit of F' changes")
                    compare(got, ref, d, K, (kind, item_rows, blocks, per_cu))
                    if per_item is None:
                        per_item = got
                    assert np.array_equal(bits(got[0]), bits(per_item[0])) and got[2] == per_item[2], (item_rows, blocks, per_cu)
    finally:
        dm.close()


# ---- chains, flags, the kernel without logarithms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 5])
def test_six_steps_in_a_chain(dev, fmh_opts, K):
    d, _, _ = R.simulate(65, 1100, K, seed=11)
    d = d[R.tracks(d)[0]][:1030]
    x = np.zeros((d.shape[0], 2 * 65), dtype=np.uint8)
    x[:, 0::2], x[:, 1::2] = (d >= 1) & (d <= 2), d == 2
    called = np.repeat(d <= 2, 2, axis=1)
    assert R.tracks(d)[4] == 1030
    fmh_opts.setenv("FMH_ADMIX_ITEM_ROWS", "256")
    dm = upload(dev, x, called, 1, True, ploidy=2)
    try:
        with dev.AdmixImage(dm) as image:
            assert image.m == 1030
            q, f = state(65, 1030, K, seed=2)
            for s in range(6):
                got = dev.admix_step(image, q, f, fill=np.nan)
                compare(got, R.step(d, q, f), d, K, ("chain", K, s))  # the oracle's step of the DEVICE's previous state
                q, f = got[0], got[1]
    finally:
        dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_flags_and_the_kernel_without_logarithms(dev, kind):
    max_allele, missing = KINDS[kind]
    n = 33
    x, called = cohort(700, 2 * n, max_allele, missing, seed=14)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        for K in (2, 5, 9, 16):
            both, d, (q, f) = check(dev, dm, x, called, (kind, "flags", K), K)
            with dev.AdmixImage(dm) as image:
                plain = dev.admix_step(image, q, f, loglik=False, fill=np.nan)
                assert plain[2] is None and np.array_equal(bits(plain[0]), bits(both[0])) and np.array_equal(bits(plain[1]), bits(both[1])), K
                only_q = dev.admix_step(image, q, f, update_f=False, fill=np.nan)
                only_f = dev.admix_step(image, q, f, update_q=False, fill=np.nan)
                neither = dev.admix_step(image, q, f, update_q=False, update_f=False, fill=np.nan)
                assert np.array_equal(bits(only_q[1]), bits(f)) and np.array_equal(bits(only_q[0]), bits(both[0])), K
                assert np.array_equal(bits(only_f[0]), bits(q)) and np.array_equal(bits(only_f[1]), bits(both[1])), K
                assert np.array_equal(bits(neither[0]), bits(q)) and np.array_equal(bits(neither[1]), bits(f)), K
                assert only_q[2] == both[2] == only_f[2] == neither[2], K
    finally:
        dm.close()


def test_no_usable_row_and_refusals(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u32 = lambda *v: np.array(v, dtype=np.uint32)

    def create(m=dm, samples=None, n=8, r0=0, rc=40, out=True):
        h = C.c_void_p()
        status = lib.fmh_admix_create(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None, C.byref(h) if out else None, None)
        if h.value:
            lib.fmh_admix_destroy(h)
        return status

    try:
        invalid = [create(m=None), create(out=False), create(n=0), create(n=9), create(samples=u32(0, 8), n=2), create(samples=u32(3, 3), n=2),
                   create(samples=u32(4, 2), n=2), create(r0=41, rc=0), create(r0=1, rc=40), create(r0=0, rc=41)]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert create(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert create(m=haploid, n=99) == _abi.FMH_ERR_INVALID  # the samples and the rows before the ploidy
        assert create(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        fmh_opts.setenv("FMH_ADMIX_BUDGET_BYTES", "100")
        assert create() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_ADMIX_BUDGET_BYTES" in lib.fmh_last_error()
        fmh_opts.reset()
        # no kept row, and no usable row: a handle with m = 0 whose step copies Q
        for kw in (dict(row_begin=3, row_count=0), dict(keep=np.zeros(40, dtype=np.uint8))):
            with dev.AdmixImage(dm, **kw) as image:
                assert image.m == 0 and image.n == 8 and not image.sample_sites.any()
                q = state(8, 0, 3, seed=1)[0]
                q1, f1, ll = dev.admix_step(image, q, np.zeros((0, 3)), fill=np.nan)
                assert np.array_equal(bits(q1), bits(q)) and f1.shape == (0, 3) and ll == 0.0
        with dev.AdmixImage(dm) as image:
            q, f = state(8, image.m, 2, seed=1)
            bufs = [dev.DeviceBuffer.from_numpy(dm.device, a) for a in (q, f, q, f)]
            step = lambda K=2, a=bufs[0].ptr, b=bufs[1].ptr, c=bufs[2].ptr, d=bufs[3].ptr, flags=3, h=image._h: lib.fmh_admix_step(h, K, a, b, c, d, None, flags, None)
            invalid = [step(h=None), step(K=0), step(K=17), step(a=None), step(b=None), step(c=None), step(d=None), step(c=bufs[0].ptr), step(d=bufs[1].ptr),
                       step(flags=4)]
            assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
            fmh_opts.setenv("FMH_ADMIX_BUDGET_BYTES", "100")
            assert step() == _abi.FMH_ERR_UNSUPPORTED and b"FMH_ADMIX_BUDGET_BYTES" in lib.fmh_last_error()
            fmh_opts.reset()
            assert np.array_equal(bufs[2].to_numpy(np.float64, q.size), q.ravel()), "a refused call wrote nothing"
            assert step() == 0
        check(dev, dm, x, called, "after the refusals", 2)
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_a_second_stream_and_two_host_threads(dev, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n, K = 70, 5
    x, called = cohort(600, 2 * n, max_allele, missing, seed=10)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    streams = [torch.cuda.Stream() for _ in range(2)]
    handles = [C.c_void_p(s.cuda_stream) for s in streams]
    assert all(h.value for h in handles), "streams of their own, not the NULL stream"
    try:
        on_stream, d, (q, f) = check(dev, dm, x, called, (kind, "on a stream"), K, stream=handles[0], pre=True)
        plain, _, _ = check(dev, dm, x, called, (kind, "NULL stream"), K)
        assert np.array_equal(bits(on_stream[0]), bits(plain[0])) and np.array_equal(bits(on_stream[1]), bits(plain[1])) and on_stream[2] == plain[2]
        with dev.AdmixImage(dm) as image:
            results = [None, None]

            def work(slot):
                results[slot] = [dev.admix_step(image, q, f, fill=np.nan, stream=handles[slot]) for _ in range(4)]

            threads = [threading.Thread(target=work, args=(slot,)) for slot in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            for slot in range(2):
                for got in results[slot]:
                    assert np.array_equal(bits(got[0]), bits(plain[0])) and np.array_equal(bits(got[1]), bits(plain[1])) and got[2] == plain[2], slot
        for s in streams:
            s.synchronize()
    finally:
        dm.close()


# ---- through `import ferromic` ----------------------------------------------------------------------------------------------------------------
def population(fm, d):
    """A from_numpy Population and the matching allele table of a dosage table [rows][n]."""
    rows, n = d.shape
    x = np.zeros((rows, 2 * n), dtype=np.uint8)
    x[:, 0::2], x[:, 1::2] = (d >= 1) & (d <= 2), d == 2
    called = np.repeat(d <= 2, 2, axis=1)
    geno = np.where(called, x, -1).astype(np.int8).reshape(rows, n, 2)
    positions = np.arange(rows, dtype=np.int64) * 5 + 3
    haps = [(s, side) for s in range(n) for side in (0, 1)]
    return fm.Population.from_numpy("p", geno, positions, haps, 5 * rows + 10), x, called, positions


def test_python_surface_is_the_unrolled_steps(dev, fm):
    d = R.simulate(33, 400, 4, seed=21)[0]
    d[5] = 0   # a row that is not usable
    d[9] = 3
    pop, x, called, positions = population(fm, d)
    usable, c, a, sites, m = R.tracks(d)
    K = 4
    q0, f0 = state(33, m, K, seed=3)
    full = np.full((d.shape[0], K), 0.5)
    full[usable] = f0
    dm = upload(dev, x, called, 1, True, ploidy=2)
    try:
        with dev.AdmixImage(dm) as image:
            # five plain steps
            q, f, trace = q0, f0, []
            for _ in range(5):
                q, f, ll = dev.admix_step(image, q, f)
                trace.append(ll)
            fit = pop.admixture(K, init=(q0, full), accelerate=False, tol=0, max_steps=5)
            assert isinstance(fit, fm.Admixture) and (fit.steps, fit.cycles, fit.accepted, fit.converged, fit.k) == (5, 0, 0, False, K)
            assert np.array_equal(bits(fit.q), bits(q)) and np.array_equal(bits(fit.frequencies[usable]), bits(f)) and np.isnan(fit.frequencies[~usable]).all()
            assert np.array_equal(fit.trace, trace) and fit.log_likelihood == dev.admix_step(image, q, f, update_q=False, update_f=False)[2]
            assert np.array_equal(fit.usable, usable) and fit.n_usable == m and np.array_equal(fit.called, c) and np.array_equal(fit.allele_count, a)
            assert np.array_equal(fit.sample_sites, sites) and np.array_equal(fit.positions, positions) and np.array_equal(fit.samples, np.arange(33))
            # three accelerated cycles
            s0, accepted, trace = (q0, f0), 0, []
            for _ in range(3):
                q1, f1, l0 = dev.admix_step(image, *s0)
                q2, f2, l1 = dev.admix_step(image, q1, f1)
                trace += [l0, l1]
                qa, fa, alpha = dev.admix_accelerate(s0, (q1, f1), (q2, f2))
                assert alpha >= 1.0
                q3, f3, la = dev.admix_step(image, qa, fa)
                trace.append(la)
                keep = np.isfinite(la) and la >= l1
                accepted += int(keep)
                s0 = (q3, f3) if keep else (q2, f2)
            fit = pop.admixture(K, init=(q0, full), accelerate=True, tol=0, max_steps=9)
            assert (fit.steps, fit.cycles, fit.accepted) == (9, 3, accepted)
            assert np.array_equal(bits(fit.q), bits(s0[0])) and np.array_equal(bits(fit.frequencies[usable]), bits(s0[1])) and np.array_equal(fit.trace, trace)
            # the default start is fmh_admix_start's
            fit = pop.admixture(K, seed=7, accelerate=False, tol=0, max_steps=1)
            qs, fs = dev.admix_start(c[usable], a[usable], 33, K, 7)
            q1, f1, _ = dev.admix_step(image, qs, fs)
            assert np.array_equal(bits(fit.q), bits(q1)) and np.array_equal(bits(fit.frequencies[usable]), bits(f1))
            # projection: F stays, Q moves as with update_f off
            fit = pop.admixture(K, init=(q0, None), frequencies=full, accelerate=False, tol=0, max_steps=2)
            q, f = q0, f0
            for _ in range(2):
                q, f, _ = dev.admix_step(image, q, f, update_f=False)
            assert np.array_equal(bits(fit.frequencies[usable]), bits(f0)) and np.array_equal(bits(fit.q), bits(q))
            fit = pop.admixture(K, frequencies=full, max_steps=30)
            assert np.array_equal(bits(fit.frequencies[usable]), bits(f0)) and fit.steps <= 30
        # variant records: a region, a sample list and a site mask
        records = []
        for i in range(120):
            calls = [None if d[i, s] == 3 else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(33)]
            records.append(dict(position=int(positions[i]), genotypes=calls))
        chosen = [s for s in range(33) if s % 7 != 3]
        mask = np.arange(80) % 3 != 1
        fit = fm.admixture(records, 2, samples=chosen, sites=mask, region=(int(positions[20]) - 1, int(positions[99]) + 1), max_steps=6, tol=0)
        sub = d[20:100][mask][:, chosen]
        assert np.array_equal(fit.usable, R.tracks(sub)[0]) and np.array_equal(fit.sites, np.flatnonzero(mask)) and np.array_equal(fit.positions, positions[20:100][mask])
        assert np.array_equal(fit.samples, chosen) and fit.q.shape == (len(chosen), 2) and np.all(np.abs(fit.q.sum(axis=1) - 1.0) < 1e-12)
        with pytest.raises(ValueError, match="sites has"):
            fm.admixture(records, 2, sites=np.ones(5, dtype=bool))
        with pytest.raises(ValueError, match="init's F has"):
            pop.admixture(K, init=(q0, f0[:10]))
        with pytest.raises(ValueError, match="outside"):
            pop.admixture(K, init=(q0, np.zeros_like(full)))
        with pytest.raises(ValueError, match="frequencies has"):
            pop.admixture(K, frequencies=full[:7])
    finally:
        dm.close()


def test_a_simulated_cohort_is_fitted(fm):
    """65 samples x 1 030 rows, K = 3: 300 plain steps and, separately, 60 accelerated cycles.  The trace does not fall, the final
    log-likelihood - evaluated by the oracle - is at least the simulating truth's, and the accelerated fit ends no lower than the plain one.
    All three are asserted on the oracle's own fit (its formulas in f64) first."""
    K = 3
    d, Qt, Ft = R.simulate(65, 1030, K, seed=5)
    usable, c, a, sites, m = R.tracks(d)
    truth = R.step(d, Qt, Ft[usable])[2]
    q0, f0 = R.start(c[usable], a[usable], 65, K, 0)
    bound = lambda ll: R.bounds(d, K, ll)[2]

    qp, fp, trace = R.fit_plain(d, q0, f0, 300)
    end_plain = R.step(d, qp, fp)[2]
    qc, fc, l0s, _ = R.fit_cycles(d, q0, f0, 60)
    end_cycles = R.step(d, qc, fc)[2]
    assert np.all(np.diff(trace) >= -2 * bound(trace[0])) and np.all(np.diff(l0s) >= -2 * bound(l0s[0]))
    assert end_plain >= truth and end_cycles >= end_plain - 2 * bound(end_plain)
    print(f"oracle: truth {truth:.3f}, 300 steps {end_plain:.3f}, 60 cycles {end_cycles:.3f}")

    pop = population(fm, d)[0]
    plain = pop.admixture(K, accelerate=False, tol=0, max_steps=300)
    fast = pop.admixture(K, accelerate=True, tol=0, max_steps=180)
    assert plain.steps == 300 and len(plain.trace) == 300 and fast.cycles == 60 and fast.steps <= 180 and np.array_equal(plain.usable, usable)
    assert np.all(np.diff(plain.trace) >= -2 * bound(plain.trace[0])), "the trace never falls by more than twice the bound"
    if fast.steps == 180:
        assert np.all(np.diff(fast.trace[0::3]) >= -2 * bound(fast.trace[0])), "l0 of successive cycles never falls"
    lp = R.step(d, plain.q, plain.frequencies[usable])[2]
    lf = R.step(d, fast.q, fast.frequencies[usable])[2]
    print(f"device: truth {truth:.3f}, 300 steps {lp:.3f}, 60 cycles {lf:.3f} ({fast.accepted} extrapolations kept)")
    assert abs(plain.log_likelihood - lp) <= 2 * bound(lp) and abs(fast.log_likelihood - lf) <= 2 * bound(lf)
    assert lp >= truth and lf >= truth, "the fit ends at or above the simulating truth"
    assert lf >= lp - 2 * bound(lp), "the accelerated fit ends no lower than the plain one"
