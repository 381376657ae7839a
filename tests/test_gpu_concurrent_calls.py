"""Every device statistic called from several host threads at once on one device (tests/concurrent_harness.py): each result of each round is
compared with the oracle of its own arguments, by the comparison the statistic's own module uses - array_equal on integers, bits on r^2 and
the HWE p-values, 1e-9 relative on the sweeps' regional sums.  Every oracle answer is computed on the main thread before a thread starts, and
every test asserts that calls of different threads were in flight together in every round (a binding that kept the interpreter lock would
make the module vacuous).

Which choice targets which shared piece of state:
  * eight different statistics on ONE matrix and one shared Groups handle, on the NULL stream, FMH_STREAM_PER_THREAD and a stream per thread -
    the per-device pool the calls' scratch comes from (abi.hip pool_malloc; DeviceScratch hands its blocks back when a call ends), the sweep
    leases, handles read by many threads; the matrix goes up as bit planes with junk under the uncalled entries;
  * ONE entry point in six threads whose arguments differ in content but not in length - every scratch array (member columns, focal rows,
    positions, work items, sample lists, kept rows, keep flags, weights, the f-moments' mask entries) falls in the same size class of the
    pool, so a block a thread returns goes straight to a neighbour; the six oracle answers are pairwise different, or cross-talk could hide;
  * kinship and pairwise differences of a 70-sample and a 129-sample matrix (129: a second 128-row tile) in four threads - the Gram workspace
    (Workspace::pd_planes / pd_slabs under Workspace::in_use) changes hands and has to grow between holders, with FMH_PD_PLANES_BYTES=1 over
    several row slabs per call, while a fifth thread calls fmh_device_release_scratch, which frees it and trims the pool;
  * two groups above 64 KiB of LDS on one haplotype kernel in two threads - the dynamic-LDS attribute belongs to the function, and both calls
    set it to their own size before they launch;
  * refusals in one thread beside good calls in another - fmh_last_error is thread-local; options changed by one thread while four launch -
    the options are atomics that a call reads once, and no result depends on them;
  * a fresh ferromic.Population and two with_haplotypes children in eight threads - the first uploads, lazy conversions and cached summaries of
    the Python module happen under contention.
Shapes are the smallest that reach that state; three rounds; at most eight threads."""

import functools
import math

import numpy as np
import pytest

from oracle import dense as D
from oracle import ferromic_ref as R
from tests import ehh_ref, fstat_ref, hap_ref, kinship_ref, ld_ref, qc_ref, sfs_ref
from tests import helpers as H
from tests.concurrent_harness import run_workers
from tests.test_gpu_ehh import assert_equal as assert_ehh_equal
from tests.test_gpu_ehh import assert_python_equal as assert_python_ehh_equal
from tests.test_gpu_ehh import mosaic_cohort
from tests.test_gpu_fstat import assert_estimate, assert_moments_equal
from tests.test_gpu_hap import assert_equal as assert_hap_equal
from tests.test_gpu_hap import assert_python_equal as assert_python_hap_equal
from tests.test_gpu_hap import largest_cohort
from tests.test_gpu_kinship import assert_kinship
from tests.test_gpu_kinship import preconditions as kinship_preconditions
from tests.test_gpu_qc import assert_bitwise, assert_qc
from tests.test_gpu_scale_pairwise import _same as assert_same_matrix
from tests.test_gpu_sfs import KINDS, assert_sfs_equal, cohort, missing_words, upload
from tests.test_sfs_cpu import sum_bound

pytestmark = pytest.mark.gpu

ROUNDS = 3
TIMEOUT_S = 120   # a cap that keeps a hang from blocking the run, not a performance figure
ROWS, COLS, SAMPLES = 600, 130, 65
ORACLE_THREADS = 16


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
STREAMS = ["null", "per-thread", "own"]


def stream_handles(kind, count):
    """(one handle per worker, whatever has to stay alive while they are used)."""
    from ferromic_amd import _abi

    if kind == "null":
        return [None] * count, None
    if kind == "per-thread":
        return [_abi.STREAM_PER_THREAD] * count, None
    import torch

    streams = [torch.cuda.Stream() for _ in range(count)]
    handles = [s.cuda_stream for s in streams]
    assert all(handles) and len(set(handles)) == count, "streams of their own, not the NULL stream"
    return handles, streams


# ---- workers: one statistic, its arguments, its oracle answer -------------------------------------------------------------------------------
class Worker:
    """call(stream) makes the device call(s); check(result) compares with `ref`, the oracle's answer for exactly these arguments."""

    def __init__(self, name, call, check, ref):
        self.name, self.call, self.check, self.ref = name, call, check, ref

    def on(self, stream):
        return (self.name, lambda: self.call(stream), self.check)


def fingerprint(ref):
    """The bytes of an oracle answer, whatever its shape: what 'pairwise different' compares."""
    if isinstance(ref, dict):
        return b"".join(fingerprint(ref[k]) for k in sorted(ref))
    if isinstance(ref, (tuple, list)):
        return b"".join(fingerprint(r) for r in ref)
    if ref is None:
        return b"-"
    return np.ascontiguousarray(ref).tobytes()


def run(workers, streams=None, rounds=ROUNDS):
    streams = streams if streams is not None else [None] * len(workers)
    report = run_workers([w.on(s) for w, s in zip(workers, streams)], rounds=rounds, timeout_s=TIMEOUT_S)
    print(f"{len(workers)} threads, overlapping pairs of calls per round: {report.overlaps}")
    report.assert_ok()
    return report


def group(dev, dm, *masks):
    return dev.Groups(dm, np.stack([np.asarray(m) for m in masks]).astype(np.uint8))


def rows_of(x, called, row_begin, row_count):
    return x[row_begin:row_begin + row_count], None if called is None else called[row_begin:row_begin + row_count]


def ld_band_worker(dev, dm, g, x, called, mask, band, threshold, row_begin=0, row_count=None, name="ld_band"):
    rows = x.shape[0] - row_begin if row_count is None else row_count
    ref = ld_ref.band(x, called, mask, row_begin, rows, row_begin + rows, band, threshold)

    def check(got):
        for key in ("n_ab", "n_joint", "site_n", "site_alt"):
            assert np.array_equal(getattr(got, key), ref[key]), (name, key)
        H.assert_bits_equal(got.r2.reshape(-1), ref["r2"].reshape(-1), name + " r2")
        assert got.over.shape == ref["over"].shape and np.array_equal(got.over, ref["over"]), (name, "over")

    return Worker(name, lambda s: dev.ld_band(dm, g, band, threshold, row_begin, rows, stream=s), check, ref)


def ld_prune_worker(dev, dm, g, x, called, mask, window, threshold, chunk_rows, name="ld_prune"):
    rows = x.shape[0]
    ref = ld_ref.greedy_from_r2(ld_ref.band(x, called, mask, 0, rows, rows, window, threshold)["r2"], threshold)
    assert 0 < ref.sum() < rows, "the pruning keeps some rows and drops some"

    def check(got):
        assert got.dtype == bool and np.array_equal(got, ref), name

    return Worker(name, lambda s: dev.ld_prune(dm, g, window, threshold, chunk_rows=chunk_rows, stream=s), check, ref)


def sfs_worker(dev, dm, g, x, called, mask, windows, name="sfs"):
    ref = sfs_ref.sfs(x, called, mask, windows)
    assert ref[0][:, 1:-1].any(), "interior bins are hit"
    return Worker(name, lambda s: dev.sfs(dm, g, windows, stream=s), lambda got: assert_sfs_equal(got, ref, name), ref)


def sfs_joint_worker(dev, dm, g2, x, called, mask0, mask1, row_begin, row_count, name="sfs_joint"):
    ref = sfs_ref.sfs_joint(x, called, mask0, mask1, row_begin, row_count)

    def check(got):
        assert got.counts.dtype == np.uint64 and np.array_equal(got.counts, ref[0]), name
        assert (got.multiallelic, got.incomplete) == ref[1:], name

    return Worker(name, lambda s: dev.sfs_joint(dm, g2, row_begin, row_count, stream=s), check, ref)


def hap_worker(dev, dm, g, x, called, mask, windows, name="haplotype_windows"):
    ref = hap_ref.windows(x, called, mask, windows)
    return Worker(name, lambda s: dev.haplotype_windows(dm, g, windows, partition=True, stream=s, fill=0xA5),
                  lambda got: assert_hap_equal(got, ref, name), ref)


def ehh_worker(dev, dm, g, x, called, mask, focal, name="ehh_scan", **kw):
    ref = ehh_ref.scan(x, called, mask, focal, **kw)
    return Worker(name, lambda s: dev.ehh_scan(dm, g, focal, stream=s, fill=0xC3, **kw), lambda got: assert_ehh_equal(got, ref, name), ref)


def fstat_worker(dev, dm, x, called, masks, blocks, name="fstat_moments"):
    ref = fstat_ref.moments(x, called, masks, blocks)
    assert ref[0][:, 0].any(), "some block has usable rows"
    return Worker(name, lambda s: dev.fstat_moments(dm, masks, blocks, stream=s), lambda got: assert_moments_equal(got, ref, name), ref)


def kinship_worker(dev, dm, x, called, samples=None, row_begin=0, row_count=None, keep=None, name="kinship_counts", ref=None):
    rows = x.shape[0] - row_begin if row_count is None else row_count
    if ref is None:
        ref = kinship_ref.tables(*rows_of(x, called, row_begin, rows), samples, keep)
    kept = rows if keep is None else int(np.count_nonzero(keep))

    def check(got):
        for table, r in zip(dev.KINSHIP_TABLES, ref):
            g = getattr(got, table)
            assert g.dtype == np.uint64 and g.shape == r.shape and np.array_equal(g, r), (name, table, np.argwhere(g != r)[:4].tolist())
        assert got.kept_rows == kept, name

    return Worker(name, lambda s: dev.kinship_counts(dm, samples=samples, row_begin=row_begin, row_count=rows, keep=keep, stream=s), check, ref)


def qc_worker(dev, dm, x, called, samples=None, row_begin=0, row_count=None, keep=None, weights=None, name="genotype_counts"):
    """fmh_genotype_counts, then fmh_hwe_exact of the site counts it returned."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    xs, cs = rows_of(x, called, row_begin, rows)
    site = qc_ref.site_tracks(xs, cs, samples)
    table = qc_ref.sample_tables(xs, cs, samples, keep)
    weighted = None if weights is None else qc_ref.weighted_called(xs, cs, weights, samples, keep)
    p = qc_ref.hwe(*site)
    ref = (site, table, weighted, p)

    def call(s):
        got = dev.genotype_counts(dm, samples=samples, row_begin=row_begin, row_count=rows, keep=keep, weights=weights, stream=s, fill=0xA5)
        return got, dev.hwe_exact(dm.device, got.site["hom_ref"], got.site["het"], got.site["hom_alt"], stream=s)

    def check(result):
        got, got_p = result
        for cls, r in zip(dev.QC_CLASSES, site):
            assert got.site[cls].dtype == np.uint32 and np.array_equal(got.site[cls], r), (name, "site", cls)
        for cls, r in zip(dev.QC_CLASSES, table):
            assert got.sample[cls].dtype == np.uint64 and np.array_equal(got.sample[cls], r), (name, "sample", cls)
        if weights is not None:
            assert np.array_equal(got.sample["weighted_called"], weighted), (name, "weighted")
        assert got.kept_rows == (rows if keep is None else int(np.count_nonzero(keep))), name
        assert_bitwise(got_p, p, name + " hwe")

    return Worker(name, call, check, ref)


def host_layout(x, called):
    """(u8 [rows][cols] with zeros at the uncalled entries, the missing words or None)."""
    if called is None:
        return np.ascontiguousarray(x), None
    return np.where(called, x, 0).astype(np.uint8), missing_words(called)


def pairwise_worker(dev, dm, x, called, max_allele, name="pairwise_differences"):
    data, words = host_layout(x, called)
    n = x.shape[1] // 2
    ref = D.pairwise_differences(data, words, x.shape[0], x.shape[1], 2, n, max_allele, ORACLE_THREADS)

    def check(got):
        assert_same_matrix(got[0], ref[0], name + " diff")
        assert_same_matrix(got[1], ref[1], name + " both")

    return Worker(name, lambda s: dev.pairwise_differences(dm, n, stream=s), check, ref)


def sweeps_worker(dev, dm, g2, x, called, h1, h2, name="hudson_sweep+population_summaries"):
    """fmh_hudson_sweep and fmh_population_summaries by the dense formulas, as tests/test_gpu_device_parity.py compares them: per-site records
    bit for bit, integers equal, regional sums within 1e-9 relative."""
    data, words = host_layout(x, called)
    rows, samples = x.shape[0], x.shape[1] // 2
    m = R.DenseGenotypeMatrix(bytes(data.reshape(-1)), None if words is None else [int(w) for w in words], rows, samples, 2, int(data.max()))
    off = [R.dense_membership_offsets(m, h) for h in (h1, h2)]
    sites = R.dense_hudson_sites(m, [R.Variant(7 * i, None) for i in range(rows)], off[0], off[1])
    L = 10 * rows + 7
    ref = dict(sites=sites, sums=R.hudson_component_sums(sites), dxy=R.calculate_dxy_dense(m, off[0], off[1], L),
               seg=[R.count_segregating_sites_dense(m, o) for o in off], pi=[R.calculate_pi_dense(m, o, L) for o in off])
    tracks = dict(fst="fst", dxy="d_xy", pi1="pi_pop1", pi2="pi_pop2", num="num_component", den="den_component")
    assert any(s.fst is not None for s in sites) and len({s.n1_called for s in sites}) > (1 if called is not None else 0)

    def call(s):
        return dev.hudson_sweep(dm, g2, dev.FORMULA_DENSE, stream=s), dev.population_summaries(dm, g2, dev.FORMULA_DENSE, stream=s)

    def check(result):
        hs, ps = result
        for key, attr in tracks.items():
            H.assert_bits_equal(hs.sites[key], [H.opt(getattr(s, attr)) for s in sites], name + " " + key)
        assert np.array_equal(hs.sites["called"][0], np.array([s.n1_called for s in sites], dtype=np.uint32)), name
        assert np.array_equal(hs.sites["called"][1], np.array([s.n2_called for s in sites], dtype=np.uint32)), name
        assert H.rel_close(hs.totals["site_num_sum"], ref["sums"][0]) and H.rel_close(hs.totals["site_den_sum"], ref["sums"][1]), name
        assert hs.totals["sites_with_components"] == sum(1 for s in sites if s.num_component is not None), name
        assert H.rel_close(hs.totals["site_dxy_sum"] / (L - hs.totals["site_dxy_skipped"]), ref["dxy"]), name
        for p in range(2):
            assert ps.totals[p]["segregating_sites"] == ref["seg"][p], (name, p)
            assert H.rel_close(ps.totals[p]["pi_sum"] / (L - ps.totals[p]["uncallable_sites"]), ref["pi"][p]), (name, p)
            assert np.array_equal(ps.called[p], hs.sites["called"][p]), (name, p)

    return Worker(name, call, check, ref)


def both(name, first, second):
    """Two workers' calls one after the other in one thread."""
    return Worker(name, lambda s: (first.call(s), second.call(s)), lambda got: (first.check(got[0]), second.check(got[1])), (first.ref, second.ref))


# ---- 1. every statistic at once on one matrix -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_cohort(kind):
    """The matrix of parts 1 and 2: a founder mosaic (so that the haplotype scans walk) with the kind's upper alleles and missing calls, and
    the masks, lists and windows the workers take."""
    x, called, positions = mosaic_cohort(ROWS, COLS, kind)
    rng = np.random.default_rng(20 + KINDS[kind][0])
    masks = rng.random((5, COLS)) < 0.5
    masks[np.arange(5), rng.integers(COLS, size=5)] = True
    seventy = rng.random(COLS) < 0.7
    samples = np.sort(rng.choice(SAMPLES, size=40, replace=False)).astype(np.uint32)
    if samples[-1] == samples.size - 1:
        samples[-1] += 1
    keep = rng.random(ROWS) < 0.6
    return dict(x=x, called=called, positions=positions, seventy=seventy, masks=masks, samples=samples, keep=keep)


def all_statistics(dev, dm, kind, handles):
    """The eight workers of part 1 and the handles to close afterwards."""
    c = shared_cohort(kind)
    x, called, positions, seventy, masks = c["x"], c["called"], c["positions"], c["seventy"], c["masks"]
    max_allele = KINDS[kind][0]
    g70 = group(dev, dm, seventy)
    g_joint = group(dev, dm, seventy, masks[0])
    h1 = H.haps_for_samples(range(0, 32))
    h2 = H.haps_for_samples(range(32, 64))   # the last sample is in neither group
    g_pair = dev.Groups.from_haplotype_lists(dm, [h1, h2])
    handles += [g70, g_joint, g_pair]
    windows = [(0, ROWS), (100, 350), (7, 7), (599, 600), (250, 251), (300, 600)]
    kinship_preconditions(kind, x, called, c["samples"])
    return [
        ld_band_worker(dev, dm, g70, x, called, seventy, 70, 0.3),
        ld_prune_worker(dev, dm, g70, x, called, seventy, 50, 0.3, 77),
        both("sfs+sfs_joint", sfs_worker(dev, dm, g70, x, called, seventy, windows),
             sfs_joint_worker(dev, dm, g_joint, x, called, seventy, masks[0], 0, ROWS)),
        hap_worker(dev, dm, g70, x, called, seventy, windows),
        ehh_worker(dev, dm, g70, x, called, seventy, list(range(4, ROWS, 41)), positions=positions, min_ehh=(1, 20), max_extent=60, curve=True),
        fstat_worker(dev, dm, x, called, masks[1:5], [(b, min(b + 97, ROWS)) for b in range(0, ROWS, 97)]),
        both("kinship_counts+genotype_counts+hwe_exact", kinship_worker(dev, dm, x, called, c["samples"], keep=c["keep"]),
             qc_worker(dev, dm, x, called, c["samples"])),
        both("pairwise_differences+sweeps", pairwise_worker(dev, dm, x, called, max_allele), sweeps_worker(dev, dm, g_pair, x, called, h1, h2)),
    ]


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_every_statistic_at_once(dev, kind, stream):
    c = shared_cohort(kind)
    dm = upload(dev, c["x"], c["called"], KINDS[kind][0], planes=True, ploidy=2)
    handles = []
    try:
        workers = all_statistics(dev, dm, kind, handles)
        assert len(workers) == 8
        streams, alive = stream_handles(stream, len(workers))
        try:
            run(workers, streams)
        finally:
            for s in alive or ():
                s.synchronize()
    finally:
        for h in handles:
            h.close()
        dm.close()


# ---- 2. one entry point, different arguments in every thread -----------------------------------------------------------------------------------
ENTRY_POINTS = ["ehh_scan", "haplotype_windows", "sfs", "fstat_moments", "genotype_counts", "kinship_counts", "ld_band"]
THREADS = 6


def same_size_masks(rng, count, members):
    masks = np.zeros((count, COLS), dtype=bool)
    for m in masks:
        m[rng.choice(COLS, size=members, replace=False)] = True
    return masks


def varied_workers(dev, dm, entry, handles):
    """Six workers of one entry point.  What differs between them is content only: every list, mask and range has the same length in all six,
    so every scratch array of the six calls is of one pool size class."""
    c = shared_cohort("multi3-missing")
    x, called, positions = c["x"], c["called"], c["positions"]
    rng = np.random.default_rng(len(entry))
    masks = same_size_masks(rng, THREADS, 61)
    workers = []
    for t in range(THREADS):
        name = f"{entry}[{t}]"
        begin = 10 * t + 3   # a row range of 520 rows, elsewhere in every thread
        if entry in ("ehh_scan", "haplotype_windows", "sfs", "ld_band"):
            g = group(dev, dm, masks[t])
            handles.append(g)
        if entry == "ehh_scan":
            focal = np.sort(rng.choice(np.arange(begin, begin + 520), size=14, replace=False))
            workers.append(ehh_worker(dev, dm, g, x, called, masks[t], focal, name, row_begin=begin, row_end=begin + 520, positions=positions,
                                      min_ehh=(1, 20), max_extent=40, curve=True))
        elif entry == "haplotype_windows":
            starts = rng.choice(ROWS - 60, size=9, replace=False)
            workers.append(hap_worker(dev, dm, g, x, called, masks[t], [(int(b), int(b) + 30) for b in starts], name))
        elif entry == "sfs":
            starts = rng.choice(ROWS - 200, size=5, replace=False)
            workers.append(sfs_worker(dev, dm, g, x, called, masks[t], [(int(b), int(b) + 150) for b in starts], name))
        elif entry == "fstat_moments":
            four = same_size_masks(rng, 4, 30)
            starts = rng.choice(ROWS - 100, size=7, replace=False)
            workers.append(fstat_worker(dev, dm, x, called, four, [(int(b), int(b) + 90) for b in starts], name))
        elif entry in ("genotype_counts", "kinship_counts"):
            samples = np.sort(rng.choice(SAMPLES - 1, size=33, replace=False)).astype(np.uint32)
            samples[-1] = SAMPLES - 1   # never the identity list: the list is uploaded
            keep = np.zeros(520, dtype=bool)
            keep[rng.choice(520, size=300, replace=False)] = True   # the same number of kept rows everywhere
            if entry == "genotype_counts":
                weights = rng.integers(0, 1 << 32, size=520, dtype=np.uint64).astype(np.uint32)
                workers.append(qc_worker(dev, dm, x, called, samples, begin, 520, keep, weights, name))
            else:
                workers.append(kinship_worker(dev, dm, x, called, samples, begin, 520, keep, name))
        elif entry == "ld_band":
            workers.append(ld_band_worker(dev, dm, g, x, called, masks[t], 33, 0.2, begin, 520, name))
    return workers


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_same_entry_point_in_every_thread(dev, entry):
    from ferromic_amd import _abi

    c = shared_cohort("multi3-missing")
    dm = upload(dev, c["x"], c["called"], 3, planes=True, ploidy=2)
    handles = []
    try:
        workers = varied_workers(dev, dm, entry, handles)
        prints = [fingerprint(w.ref) for w in workers]
        assert len(workers) == THREADS and len(set(prints)) == THREADS, "the six oracle answers are pairwise different"
        run(workers, [_abi.STREAM_PER_THREAD] * THREADS)
    finally:
        for h in handles:
            h.close()
        dm.close()


# ---- 3. the Gram workspace between kinship and pairwise differences --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram_cohorts():
    out = []
    for rows, cols in ((300, 140), (1300, 258)):
        x, called = cohort(rows, cols, 3, True, seed=5)
        out.append((x, called, kinship_preconditions("multi3-missing", x, called)))
    return out


@pytest.mark.parametrize("planes_bytes", [None, "1"], ids=["default", "row-slabs"])
def test_gram_workspace_changes_hands(dev, fmh_opts, planes_bytes):
    """kinship(A), pairwise(B), kinship(B), pairwise(A): A is 300 rows x 70 samples, B 1 300 rows x 129 samples, so the planes buffer a call
    finds is too small or larger than it needs, by turns.  FMH_PD_PLANES_BYTES=1: one K block per row slab, several slabs per call.
    fmh_device_release_scratch: the header allows it while other calls are in flight (it frees the Gram workspace under the lock a Gram call
    holds for its whole length, and only idle blocks of the pool), so a fifth thread calls it once a round: it must change nobody's answer."""
    from ferromic_amd import _abi

    lib = _abi.load()
    if planes_bytes is not None:
        fmh_opts.setenv("FMH_PD_PLANES_BYTES", planes_bytes)   # before any thread starts
    (xa, ca, ref_a), (xb, cb, ref_b) = gram_cohorts()
    a, b = upload(dev, xa, ca, 3, ploidy=2), upload(dev, xb, cb, 3, ploidy=2)
    try:
        release = Worker("release_scratch", lambda s: lib.fmh_device_release_scratch(a.device), lambda status: _abi.check(status), None)
        workers = [kinship_worker(dev, a, xa, ca, name="kinship(A)", ref=ref_a), pairwise_worker(dev, b, xb, cb, 3, "pairwise(B)"),
                   kinship_worker(dev, b, xb, cb, name="kinship(B)", ref=ref_b), pairwise_worker(dev, a, xa, ca, 3, "pairwise(A)"), release]
        run(workers, [_abi.STREAM_PER_THREAD] * len(workers))
    finally:
        a.close()
        b.close()


# ---- 4. two group sizes above 64 KiB of LDS at once -----------------------------------------------------------------------------------------
def hap_lds_bytes(n):
    """hap_lds_bytes of hap_kernels.hpp, restated (the library exposes no launch figures): a head of 128 words, one label word per member
    padded to four, and three words per 16 members, each padded to four - 4 bytes each."""
    pad4 = lambda v: (v + 3) & ~3
    return (128 + pad4(n) + 3 * pad4((n + 15) // 16)) * 4


def first_group_above(limit):
    n = 1
    while hap_lds_bytes(n) <= limit:
        n += 1
    return n


@pytest.mark.parametrize("entry", ["ehh_scan", "haplotype_windows"])
def test_two_large_groups_at_once(dev, entry):
    """Two groups of one kernel instantiation whose dynamic LDS differs and is above 64 KiB for both - the largest group the kernel takes
    (34 304 members: 163 456 bytes) and the smallest group above 64 KiB plus 1 000 members (13 689 + 1 000: 70 320 bytes) - launched from two
    threads.  The launcher sets hipFuncAttributeMaxDynamicSharedMemorySize to its own call's bytes before it launches; were the attribute enforced at launch
    and the two set / launch pairs interleaved, the larger call would come back with FMH_ERR_HIP."""
    from ferromic_amd import _abi

    cap = dev.ehh_max_members() if entry == "ehh_scan" else dev.haplotype_max_members()
    smaller = first_group_above(64 << 10) + 1000
    assert 64 << 10 < hap_lds_bytes(smaller) < hap_lds_bytes(cap) <= 160 << 10 and smaller < cap // 2
    x = largest_cohort(cap)
    rng = np.random.default_rng(4)
    largest = np.ones(cap + 1, dtype=bool)
    largest[cap // 3] = False
    some = np.zeros(cap + 1, dtype=bool)
    some[rng.choice(cap + 1, size=smaller, replace=False)] = True
    dm = upload(dev, x, None, 1, planes=True, ploidy=1)
    handles = [group(dev, dm, largest), group(dev, dm, some)]
    try:
        if entry == "ehh_scan":
            workers = [ehh_worker(dev, dm, handles[0], x, None, largest, [0, 12, 23], "ehh_scan[cap]"),
                       ehh_worker(dev, dm, handles[1], x, None, some, [3, 11, 20], f"ehh_scan[{smaller}]")]
        else:
            workers = [hap_worker(dev, dm, handles[0], x, None, largest, [(0, 24), (0, 3), (20, 21)], "haplotype_windows[cap]"),
                       hap_worker(dev, dm, handles[1], x, None, some, [(0, 24), (2, 9), (20, 21)], f"haplotype_windows[{smaller}]")]
        assert fingerprint(workers[0].ref) != fingerprint(workers[1].ref)
        run(workers, [_abi.STREAM_PER_THREAD] * 2)
    finally:
        for h in handles:
            h.close()
        dm.close()


# ---- 5. through `import ferromic` -------------------------------------------------------------------------------------------------------------
def python_workers(fm, x, called, positions, pops, masks, haps):
    """Eight workers over one Population and its two with_haplotypes children (pops = base, p1, p2; masks / haps likewise)."""
    base, p1, p2 = pops
    m0, m1, m2 = masks
    rows = x.shape[0]
    every = list(range(rows))
    n0, n1, n2 = (int(m.sum()) for m in masks)

    r2 = ld_ref.band(x, called, m0, 0, rows, rows, 33, 0.0)["r2"]
    pruned = ld_ref.greedy_from_r2(r2, 0.2)

    def check_ld(got):
        H.assert_bits_equal(got[0].reshape(-1), r2.reshape(-1), "Population.ld_r2")
        assert got[1].dtype == bool and np.array_equal(got[1], pruned)

    spectrum = sfs_ref.sfs(x, called, m1, [(0, rows)])
    joint = sfs_ref.sfs_joint(x, called, m1, m2, 0, rows)
    stats = sfs_ref.stats(spectrum[0][0])

    def check_sfs(got):
        one, two = got
        assert one.sample_size == n1 and np.array_equal(one.counts, spectrum[0][0])
        assert (one.multiallelic_sites, one.incomplete_sites) == (int(spectrum[1][0]), int(spectrum[2][0]))
        assert one.segregating_sites == stats["segregating_sites"]
        assert abs(one.tajimas_d - stats["tajima_d"]) <= sum_bound(n1) * (stats["pi_sum"] + stats["theta_w_sum"]) / stats["tajima_d_sd"]
        assert two.sample_sizes == (n1, n2) and np.array_equal(two.counts, joint[0]) and (two.multiallelic_sites, two.incomplete_sites) == joint[1:]

    ranges = [(r, r + 50) for r in range(0, rows - 49, 25)]
    hap = hap_ref.windows(x, called, m2, ranges)
    ihs = ehh_ref.scan(x, called, m1, every, positions=positions, min_ehh=(50_000, 1_000_000), min_core=math.ceil(0.05 * n1))
    nsl = ehh_ref.scan(x, called, m2, every, max_extent=100)

    four = np.stack([m1, m2, m0 & ~m1, m0 & ~m2])
    four_haps = [haps[1], haps[2], [h for h in haps[0] if h not in set(haps[1])], [h for h in haps[0] if h not in set(haps[2])]]
    blocks = [(r, min(r + 60, rows)) for r in range(0, rows, 60)]
    moments = fstat_ref.moments(x, called, four, blocks)
    sizes = four.sum(axis=1).astype(np.uint64)
    block_positions = [(int(positions[b]), int(positions[e - 1])) for b, e in blocks]

    def call_f():
        fs = fm.f_statistics([base.with_haplotypes(i, h) for i, h in enumerate(four_haps)], blocks=block_positions)
        return fs, fs.f2(0, 1), fs.f3(2, 0, 1), fs.f4(0, 1, 2, 3)

    def check_f(got):
        fs, f2, f3, f4 = got
        assert np.array_equal(fs.moments, moments[0]) and np.array_equal(fs.multiallelic_sites, moments[1]) and np.array_equal(fs.incomplete_sites, moments[2])
        assert_estimate(f2, moments[0], sizes, (0, 1, 0, 1))
        assert_estimate(f3, moments[0], sizes, (2, 0, 2, 1))
        assert_estimate(f4, moments[0], sizes, (0, 1, 2, 3))

    whole = sorted({s for s, _ in haps[0]})   # the population holds both haplotypes of each of its samples

    def call_qc():
        qc = base.genotype_qc()
        sites = qc.site_filter(min_call_rate=0.95, min_maf=0.02, min_hwe_p=1e-6)
        return qc, sites, base.genotype_qc(sites=sites), base.kinship(sites=sites)

    site_ref = qc_ref.site_tracks(x, called, whole)

    def check_qc(got):
        qc, sites, restricted, kin = got
        assert_qc(qc, x, called, whole, None, "Population.genotype_qc")
        assert sites.dtype == bool and sites.shape == (rows,) and 0 < sites.sum() < rows
        assert_qc(restricted, x, called, whole, sites, "Population.genotype_qc(sites)")
        assert_kinship(kin, x, called, whole, sites, "Population.kinship(sites)")

    assert np.unique(site_ref[1]).size > 1
    data, words = host_layout(x, called)
    ref_matrix = R.DenseGenotypeMatrix(bytes(data.reshape(-1)), [int(w) for w in words], rows, x.shape[1] // 2, 2, 1)
    totals = R.aggregate_hudson_components_from_summaries(R.build_dense_population_summary(ref_matrix, haps[1]),
                                                          R.build_dense_population_summary(ref_matrix, haps[2]))
    fst = totals.numerator_sum / totals.denominator_sum

    def check_hudson(got):
        assert abs(got.fst - fst) <= 1e-9 * abs(fst), (got.fst, fst)

    plain = lambda call: (lambda s: call())
    return [
        Worker("ld_r2+ld_prune", plain(lambda: (base.ld_r2(33), base.ld_prune(33, 0.2))), check_ld, None),
        Worker("sfs+tajima", plain(lambda: (p1.site_frequency_spectrum(), fm.joint_site_frequency_spectrum(p1, p2))), check_sfs, None),
        Worker("garud_h", plain(lambda: p2.garud_h(size=50, step=25, partition=True)),
               lambda got: assert_python_hap_equal(got, hap, n2, ranges, True), None),
        Worker("ihs", plain(lambda: p1.ihs()), lambda got: assert_python_ehh_equal(got, ihs[0], None, n1, every, False), None),
        Worker("nsl", plain(lambda: p2.nsl()), lambda got: assert_python_ehh_equal(got, nsl[0], None, n2, every, True), None),
        Worker("f_statistics", plain(call_f), check_f, None),
        Worker("genotype_qc+kinship", plain(call_qc), check_qc, None),
        Worker("hudson_fst", plain(lambda: fm.hudson_fst(p1, p2)), check_hudson, None),
    ]


def test_python_threads_share_a_population_for_every_statistic(fm):
    """300 sites x 40 diploid samples with missing calls: a Population of 36 samples and two children of 18 and 17 of them, made and left
    untouched until the threads start - the first uploads, the packed image and the cached summaries come to be under contention."""
    rows, samples = 300, 40
    x, called = cohort(rows, 2 * samples, 1, True, seed=43)
    called = np.repeat(called[:, 0::2], 2, axis=1)   # a genotype is called or not as a whole
    positions = 100 + 7 * np.arange(rows)
    geno = np.where(called, x, -1).astype(np.int8).reshape(rows, samples, 2)
    rng = np.random.default_rng(43)
    chosen = sorted(int(s) for s in rng.choice(samples, size=36, replace=False))
    haps = [H.haps_for_samples(chosen), H.haps_for_samples(chosen[:18]), H.haps_for_samples(chosen[18:35])]
    masks = []
    for h in haps:
        mask = np.zeros(2 * samples, dtype=bool)
        for s, side in h:
            mask[2 * s + side] = True
        masks.append(mask)
    kinship_preconditions("missing", x, called, chosen)
    base = fm.Population.from_numpy("all", geno, positions.astype(np.int64), haps[0], int(positions[-1]) + 1)
    pops = (base, base.with_haplotypes(1, haps[1]), base.with_haplotypes(2, haps[2]))
    run(python_workers(fm, x, called, positions, pops, masks, haps))


# ---- 6. errors and options stay where they belong --------------------------------------------------------------------------------------------
def test_refusals_stay_with_their_thread(dev):
    """One thread makes only refused calls - fmh_ld_band with band 0, fmh_ehh_scan without a focal row, fmh_kinship_counts of a haploid
    matrix - a fixed 200 times each per round, while another computes fmh_ld_band and fmh_ehh_scan against the oracle.  The statuses and
    messages are those the single-threaded refusal tests pin; the computing thread never sees them.  Each thread ends every round - the
    refusing one after its 600 refusals, the computing one after its checked calls - with one more fmh_ld_band and fmh_ehh_scan of its own
    against the oracle and a synchronisation of its own stream: the calls are correct and nothing is left behind in that thread, neither a
    launch error nor a refusal's status."""
    from ferromic_amd import _abi

    lib = _abi.load()
    c = shared_cohort("multi3-missing")
    x, called, positions, seventy = c["x"], c["called"], c["positions"], c["seventy"]
    dm = upload(dev, x, called, 3, planes=True, ploidy=2)
    haploid = upload(dev, x, called, 3, planes=True, ploidy=1)
    g = group(dev, dm, seventy)
    texts = ("band is 0", "n_focal", "ploidy")

    def refuse(s):
        seen = []
        for call, status in ((lambda: dev.ld_band(dm, g, 0, stream=s), _abi.FMH_ERR_INVALID),
                             (lambda: dev.ehh_scan(dm, g, [], stream=s), _abi.FMH_ERR_INVALID),
                             (lambda: dev.kinship_counts(haploid, n_samples=4, stream=s), _abi.FMH_ERR_UNSUPPORTED)):
            for _ in range(200):
                try:
                    call()
                    seen.append((0, ""))
                except _abi.FerromicHipError as err:
                    seen.append((err.status, str(err)))
                assert seen[-1][0] == status, seen[-1]
        return seen, good_calls(s)

    def check_refused(result):
        seen, good = result
        check_good(good)
        assert len(seen) == 600
        for k, (status, text) in enumerate(seen):
            assert texts[k // 200] in text and not any(t in text for t in texts if t != texts[k // 200]), (k, text)

    band = ld_band_worker(dev, dm, g, x, called, seventy, 33, 0.2)
    scan = ehh_worker(dev, dm, g, x, called, seventy, list(range(9, ROWS, 53)), positions=positions, min_ehh=(1, 20), max_extent=60, curve=True)

    def good_calls(s):
        """In the calling thread: both statistics once more, then its own stream synchronised (a launch error left behind would show here)."""
        out = [band.call(s), scan.call(s)]   # a FerromicHipError here is a failure of the worker
        _abi.check(lib.fmh_stream_synchronize(dm.device, s))
        return out

    def check_good(out):
        band.check(out[0])
        scan.check(out[1])

    def compute(s):
        out = []
        for w in (band, scan):
            out.append(w.call(s))   # a FerromicHipError here is a failure of the worker
            last = lib.fmh_last_error().decode()
            assert not any(t in last for t in texts), f"the other thread's message in this one: {last!r}"
        return out, good_calls(s)

    def check_computed(result):
        check_good(result[0])
        check_good(result[1])

    try:
        workers = [Worker("refused", refuse, check_refused, None), Worker("computing", compute, check_computed, None)]
        run(workers, [_abi.STREAM_PER_THREAD] * 2)
        # and from two fresh threads, which share the device with whatever the first two left
        run([Worker("after-1", compute, check_computed, None), Worker("after-2", compute, check_computed, None)], [_abi.STREAM_PER_THREAD] * 2, rounds=1)
    finally:
        g.close()
        haploid.close()
        dm.close()


# Read once per call, or every use from one snapshot, by reading hap_launch.hpp (FMH_HAP_THREADS), stat_call.hpp (FMH_GRID_BLOCKS,
# FMH_GRID_PER_CU and, through item_rows_of, the item-row options of sfs.hip, fstat.hip, qc.hip) and gram_launch.hpp / pairwise.hip (gram_format, gram_row_slab, gram_plan: the FMH_PD_* ones).
OPTION_VALUES = {
    "FMH_HAP_THREADS": ["64", "256", "512", "1024", None],
    "FMH_GRID_BLOCKS": ["3", None],
    "FMH_GRID_PER_CU": ["1", None],
    "FMH_SFS_ITEM_ROWS": ["16", "100", None],
    "FMH_FSTAT_ITEM_ROWS": ["16", "100", None],
    "FMH_QC_ITEM_ROWS": ["16", None],
    "FMH_PD_KCHUNK": ["128", None],
    "FMH_PD_PLANES_BYTES": ["1", None],
    "FMH_PD_INT8": ["1", None],
    "FMH_PD_PHASED": ["0", None],
    "FMH_PD_SLABS": ["0", None],
}
OPTION_CHANGES = 30
REPEATS = 6


def test_options_change_while_others_launch(dev, fmh_opts):
    """One thread makes a fixed 30 option changes per round, each followed by a small fmh_sfs call of its own (which spreads the changes over
    the round and is itself compared); four threads run fmh_haplotype_windows, fmh_sfs, fmh_fstat_moments and fmh_kinship_counts six times per
    round against the oracle.  The header: setting an option while another thread launches is safe, and no result depends on one."""
    from ferromic_amd import _abi

    c = shared_cohort("multi3-missing")
    x, called, seventy, masks = c["x"], c["called"], c["seventy"], c["masks"]
    dm = upload(dev, x, called, 3, planes=True, ploidy=2)
    g = group(dev, dm, seventy)
    windows = [(0, ROWS), (100, 350), (7, 7), (599, 600), (300, 600)]
    plan = [(key, values[i % len(values)]) for i in range(3) for key, values in OPTION_VALUES.items()][:OPTION_CHANGES]
    assert len(plan) == OPTION_CHANGES and {key for key, _ in plan} == set(OPTION_VALUES)
    small = sfs_worker(dev, dm, g, x, called, seventy, [(40, 90)], "sfs beside the changes")

    def change(s):
        out = []
        for key, value in plan:
            (fmh_opts.setenv(key, value) if value is not None else fmh_opts.delenv(key))
            out.append(small.call(s))
        return out

    def repeated(w):
        def check(results):
            assert len(results) == REPEATS
            for r in results:
                w.check(r)
        return Worker(w.name, lambda s: [w.call(s) for _ in range(REPEATS)], check, w.ref)

    try:
        workers = [Worker("options", change, lambda out: [small.check(r) for r in out], None),
                   repeated(hap_worker(dev, dm, g, x, called, seventy, windows)),
                   repeated(sfs_worker(dev, dm, g, x, called, seventy, windows)),
                   repeated(fstat_worker(dev, dm, x, called, masks[1:5], [(b, min(b + 97, ROWS)) for b in range(0, ROWS, 97)])),
                   repeated(kinship_worker(dev, dm, x, called, c["samples"], keep=c["keep"]))]
        run(workers, [_abi.STREAM_PER_THREAD] * len(workers))
    finally:
        fmh_opts.reset()
        g.close()
        dm.close()
