"""Crossing fuzz of the core of the library - fmh_population_summaries, fmh_hudson_sweep in its three formula sets, fmh_diversity_sites,
fmh_wc_sweep / fmh_wc_sweep_many, fmh_pair_region_sweep, fmh_pairwise_differences, fmh_pca_scan_sites and fmh_pca_gram - against the C
oracle (oracle/dense.py) and numpy.

One test per seed (tests/sweep_fuzz.py draws the case; tests/test_sweep_fuzz_draws_cpu.py shows what the default seeds cover): the matrix
is made ONCE, through one of eight origins - the six of the cohort fuzz, fmh_matrix_wrap left on the caller's u8 rows, and
fmh_matrix_create under FMH_LAYOUT=bytes - with every routing option of sweep_plan.hpp drawn on its own, and every call runs on that one
matrix in turn: on a row range whose ends fall inside a 64-row tile, on a grid of one or three workgroups, on a stream of the case's own.
The references see np.where(called, x, 0) and the missing words, never the junk a plane holds under an uncalled entry or a wrapped row
holds in its padding.

Each result is compared as in that call's own file: integer tables with array_equal, per-site f64 tracks bit for bit (NaN positions
equal), regional sums with helpers.rel_close (1e-9), the Gram within the bound of tests/test_gpu_pca.py.  The probes are asserted where
the draw fixes their answer.  Afterwards the download is the cohort with zeros under the missing entries, and the caller's device blocks of
a wrapped matrix are byte for byte what was uploaded.

FERROMIC_FUZZ_SWEEP_CASES sets the number of seeds (default 96)."""

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests import sweep_fuzz as S
from tests.cohort_fuzz import stream_handle
from tests.test_gpu_pca import gram_expectation
from tests.test_gpu_pca_scan import SENTINEL_ALT, SENTINEL_FLAG
from tests.test_gpu_scale_general import check_hudson, check_wc
from tests.test_gpu_scale_sparse import SUMMARY_SUMS, TRACKS, check_fused_sites, check_fused_totals, check_hud_totals, check_hudson_sites, check_pop, unpack_fused
from tests.test_gpu_sfs import missing_words

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("FERROMIC_FUZZ_SWEEP_CASES", str(S.DEFAULT_CASES)))
# seeds that once failed, with the cause
REGRESSION_SEEDS = [
    14,  # W&C on the u8 rows of a wrapped matrix counted the padding bits of a row's last 16-bit called word into n_all: a row with no called
    70,  # entry came out NO_VARIANCE (2) instead of INSUFFICIENT (3) - sweep_kernels.hpp, called_tail16
]
THREADS = 4  # the oracle's thread count: passed, never taken from the machine
PAD = 9


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


class Cohort:
    """What the references see of the case's rows [row_begin, row_begin + row_count): zeros under the missing entries, and the words."""

    def __init__(self, case, x, called):
        r0, r1 = case.row_begin, case.row_begin + case.row_count
        self.rows, self.columns = case.row_count, case.columns
        self.everyone = np.ones(x.shape, dtype=bool) if called is None else called
        self.whole = x if called is None else np.where(called, x, 0).astype(np.uint8)
        self.whole_words = None if called is None else missing_words(called)
        self.data = np.ascontiguousarray(self.whole[r0:r1])
        self.flat = self.data.reshape(-1)
        self.mask = self.everyone[r0:r1]
        self.words = None if called is None else missing_words(np.ascontiguousarray(called[r0:r1]))

    def counts(self, masks, max_allele):
        """(called [G][rows], count of every allele [A][G][rows]) of the groups `masks`, exact in f32 products (counts below 2^24)."""
        m = masks.T.astype(np.float32)
        called = (self.mask.astype(np.float32) @ m).T.astype(np.uint32)
        per_allele = np.stack([(((self.data == a) & self.mask).astype(np.float32) @ m).T for a in range(max_allele + 1)]).astype(np.uint32)
        return called, per_allele


def check_summaries(dev, dm, case, co, stream):
    masks = case.summary
    got = dev.population_summaries(dm, dev.Groups(dm, masks), case.summaries_formula, case.row_begin, case.row_count, stream=stream)
    called, per_allele = co.counts(masks, case.max_allele)
    distinct = (per_allele > 0).sum(axis=0)
    assert got.called.dtype == np.uint32 and np.array_equal(got.called, called), "summaries: called"
    assert np.array_equal(got.alt, per_allele[1]), "summaries: alt"
    for g in range(masks.shape[0]):
        assert got.totals[g]["segregating_sites"] == int((distinct[g] >= 2).sum()), ("summaries: segregating", g)
        assert got.totals[g]["uncallable_sites"] == int((called[g] < 2).sum()), ("summaries: uncallable", g)
        assert got.totals[g]["haplotype_capacity"] == int(masks[g].sum()), ("summaries: capacity", g)


def check_hudson_sweeps(dev, dm, g2, case, co, off1, off2, stream):
    """The three formula sets.  Returns the DENSE and the SPARSE result for the fused sweep to be held against."""
    bi = case.max_allele <= 1
    r0, rows, Hc = case.row_begin, case.row_count, case.columns
    dense_exp = D.hudson_sweep_dense(co.flat, co.words, rows, Hc, case.max_allele, off1, off2, THREADS)
    dense = dev.hudson_sweep(dm, g2, dev.FORMULA_DENSE, r0, rows, stream=stream)
    check_hudson(dense, dense_exp, not bi, "Hudson, dense formulas")
    sparse_exp = D.region_sweep(co.flat, co.words, rows, Hc, case.max_allele, off1, off2, D.FORMULA_SPARSE, D.FORMULA_SPARSE, THREADS)
    sparse = dev.hudson_sweep(dm, g2, dev.FORMULA_SPARSE, r0, rows, stream=stream)
    check_hudson_sites(sparse.sites, sparse_exp, slice(0, rows), bi, "Hudson, sparse formulas")
    for p in range(2):
        check_pop(sparse.pop[p], sparse_exp.pop[p], f"Hudson, sparse formulas, population {p}")
    check_hud_totals(sparse.totals, sparse_exp.totals, bi, "Hudson, sparse formulas")
    if bi:  # the totals of the two summaries (aggregate_hudson_components_from_summaries), with no per-site track asked for
        summary = dev.hudson_sweep(dm, g2, dev.FORMULA_SUMMARY, r0, rows, want_sites=False, stream=stream)
        for k in SUMMARY_SUMS:
            assert H.rel_close(summary.totals[k], dense_exp.totals[k]), ("Hudson, summary formulas", k, summary.totals[k], dense_exp.totals[k])
        assert summary.totals["dxy_uncallable_sites"] == dense_exp.totals["dxy_uncallable_sites"], "Hudson, summary formulas"
        for p in range(2):
            for k in ("segregating_sites", "uncallable_sites"):
                assert summary.pop[p][k] == dense_exp.pop[p][k], ("Hudson, summary formulas", p, k)
            assert summary.pop[p]["haplotype_capacity"] == int(case.pair[p].sum())
    return {dev.FORMULA_DENSE: dense, dev.FORMULA_SPARSE: sparse}


def fused_sweep(dev, dm, g2, r0, rows, summary_formula, hudson_formula, stream):
    from ferromic_amd import _abi

    bufs = {k: dev.DeviceBuffer(dm.device, 16 * rows) for k in ("pi", "theta")}
    bufs.update({k: dev.DeviceBuffer(dm.device, 8 * rows) for k in TRACKS + ("alt", "called")})
    div = _abi.PairDiversitySites(bufs["pi"].ptr, bufs["theta"].ptr)
    sites = _abi.HudsonSites(*(bufs[k].ptr for k in TRACKS + ("alt", "called")))
    tot = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_pair_region_sweep(dm._h, g2._h, r0, rows, summary_formula, hudson_formula, C.byref(div), C.byref(sites), C.byref(tot), stream))
    return unpack_fused(dev, bufs, tot, rows)


def check_fused(dev, dm, g2, g1, case, co, off1, off2, separate, stream):
    bi = case.max_allele <= 1
    r0, rows, Hc = case.row_begin, case.row_count, case.columns
    sf, hf = case.fused
    fu = fused_sweep(dev, dm, g2, r0, rows, sf, hf, stream)
    what = f"fused sweep, formulas {sf}/{hf}"
    # against the oracle (whose fused sweep has the sparse Hudson formulas, or none)
    exp = D.region_sweep(co.flat, co.words, rows, Hc, case.max_allele, off1, off2, sf, hf if hf == D.FORMULA_SPARSE else -1, THREADS)
    if hf == D.FORMULA_SPARSE:
        check_fused_sites(fu, exp, slice(0, rows), bi, what)
        check_fused_totals(fu, SimpleNamespace(pop={sf: exp.pop}, hud=exp.totals), sf, bi, what)
    else:
        for p in range(2):
            H.assert_bits_equal(fu["pi"][p], exp.site_pi[p], f"site pi group {p} {what}")
            H.assert_bits_equal(fu["theta"][p], exp.site_theta[p], f"site theta group {p} {what}")
            check_pop(fu["pop"][p], exp.pop[p], f"population {p} {what}")
        assert np.array_equal(fu["sites"]["called"], exp.called), what
        assert not bi or np.array_equal(fu["sites"]["alt"], exp.alt), what
        if hf < 0:
            check_hud_totals(fu["totals"], exp.totals, bi, what)  # all zero
            assert fu["totals"]["sites_with_components"] == 0 and fu["totals"]["numerator_sum"] == 0.0 and fu["totals"]["site_num_sum"] == 0.0, what
    # against the separate calls: the same bits per site, equal integers, f64 totals to 1e-12 (another grid adds the partials in another order)
    ps = dev.population_summaries(dm, g2, sf, r0, rows, stream=stream)
    alone = D.region_sweep(co.flat, co.words, rows, Hc, case.max_allele, off1, off2, D.FORMULA_SPARSE, -1, THREADS)  # fmh_diversity_sites' totals
    for p in range(2):
        for k in ("haplotype_capacity", "segregating_sites", "uncallable_sites"):
            assert fu["pop"][p][k] == ps.totals[p][k], (what, p, k)
        assert fu["pop"][p]["pi_sum"] == pytest.approx(ps.totals[p]["pi_sum"], rel=1e-12, abs=1e-300), (what, p)
        dv = dev.diversity_sites(dm, g1[p], r0, rows, stream=stream)
        H.assert_bits_equal(fu["pi"][p], dv.pi, f"site pi group {p}, the separate call, {what}")
        H.assert_bits_equal(fu["theta"][p], dv.theta, f"site theta group {p}, the separate call, {what}")
        assert np.array_equal(dv.called, exp.called[p]) and np.array_equal(dv.distinct, exp.distinct[p]), (what, p, "diversity_sites counts")
        check_pop(dv.totals, alone.pop[p], f"diversity_sites group {p}")
    assert np.array_equal(fu["sites"]["called"], ps.called), what
    assert not bi or np.array_equal(fu["sites"]["alt"], ps.alt), what
    if hf >= 0:
        hs = separate[hf]
        for k in TRACKS:
            H.assert_bits_equal(fu["sites"][k], hs.sites[k], f"{k}, the separate call, {what}")
        for k, v in hs.totals.items():
            got = fu["totals"][k]
            if isinstance(v, int):
                assert got == v, (what, k)
            else:
                assert got == pytest.approx(v, rel=1e-12, abs=1e-300), (what, k)


def check_wc_sweeps(dev, dm, case, co, stream):
    masks = case.wc
    G, r0, rows = masks.shape[0], case.row_begin, case.row_count
    goc = np.full(case.columns, 0xFF, dtype=np.uint8)
    for g in range(G):
        goc[masks[g] != 0] = g
    exp = D.wc_sites(co.flat, co.words, rows, case.columns, goc, G, THREADS)
    w = dev.wc_sweep(dm, dev.Groups(dm, masks), r0, rows, stream=stream)
    check_wc(w, exp, f"W&C, {G} groups")
    assert np.array_equal(w.group_called, co.counts(masks, 0)[0]), "W&C: group sizes"
    wm = dev.wc_sweep_many(dm, masks, r0, rows, stream=stream)  # the counts path: the same per-site bits
    for name in ("a", "b"):
        assert np.array_equal(getattr(wm, name).view(np.uint64), getattr(w, name).view(np.uint64)), ("wc_sweep_many", name)
    assert np.array_equal(wm.state, w.state) and np.array_equal(wm.group_called, w.group_called), "wc_sweep_many"
    assert np.array_equal(wm.informative_sites, w.informative_sites), "wc_sweep_many"
    wt = dev.wc_sweep_many(dm, masks, r0, rows, sites=False, stream=stream)  # no track asked for: the sums straight from the count tables
    assert np.array_equal(wt.informative_sites, wm.informative_sites), "wc_sweep_many, no sites"
    assert np.allclose(wt.sum_a, wm.sum_a, rtol=1e-11, atol=1e-11) and np.allclose(wt.sum_b, wm.sum_b, rtol=1e-11, atol=1e-11), "wc_sweep_many, no sites"


def check_pairwise(dev, fmh_opts, dm, case, co, stream):
    n = min(case.samples, S.PAIRWISE_MAX_SAMPLES)
    exp_diff, exp_both = D.pairwise_differences(co.whole, co.whole_words, case.rows, case.columns, case.ploidy, n, case.max_allele, THREADS)
    for key, value in case.pd_set:
        fmh_opts.setenv(key, value)
    try:
        diff, both = dev.pairwise_differences(dm, n, stream=stream)
    finally:
        for key, _ in case.pd_set:
            fmh_opts.delenv(key)
    iu = np.triu_indices(n, k=1)
    assert diff.dtype == np.uint64 and np.array_equal(diff[iu], exp_diff[iu]), ("pairwise diff", case.pd_set)
    assert np.array_equal(both[iu], exp_both[iu]), ("pairwise both", case.pd_set)


def check_pca_scan(dev, dm, case, co, stream):
    from ferromic_amd import _abi

    r0, rows = case.row_begin, case.row_count
    d_alt = dev.DeviceBuffer.from_numpy(dm.device, np.full(rows + PAD, SENTINEL_ALT, dtype=np.uint32))
    d_flags = dev.DeviceBuffer.from_numpy(dm.device, np.full(rows + PAD, SENTINEL_FLAG, dtype=np.uint8))
    _abi.check(_abi.load().fmh_pca_scan_sites(dm._h, r0, rows, d_alt.ptr, d_flags.ptr, stream))
    alt, flags = d_alt.to_numpy(np.uint32, rows + PAD), d_flags.to_numpy(np.uint8, rows + PAD)
    d_alt.free()
    d_flags.free()
    exp_flags = np.where((~co.mask).any(axis=1), 1, 0) | np.where(((co.data > 1) & co.mask).any(axis=1), 2, 0)
    exp_alt = ((co.data == 1) & co.mask).sum(axis=1)
    assert np.array_equal(flags[:rows], exp_flags.astype(np.uint8)), "pca scan: flags"
    assert np.array_equal(alt[:rows], exp_alt.astype(np.uint32)), "pca scan: alt"
    assert np.all(alt[rows:] == SENTINEL_ALT) and np.all(flags[rows:] == SENTINEL_FLAG), "pca scan: written beyond row_count"


def check_pca_gram(dev, dm, case, co, stream):
    clean = co.everyone.all(axis=1) & (co.whole <= 1).all(axis=1)
    kept = np.nonzero(clean)[0].astype(np.uint64)
    if kept.size == 0:
        return
    n = case.columns
    hi, lo, _, expected, bound = gram_expectation(co.whole[kept.astype(np.int64)], n)
    got = dev.pca_gram(dm, kept, hi, lo, stream=stream)
    err = np.abs(got - expected)
    assert np.all(err <= bound), ("pca gram", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.array_equal(got, got.T), "the Gram must be exactly symmetric"


def check_probes(dev, dm, g2, g1, case):
    pairs = ((g2, dev.SWEEP_SUMMARY), (g2, dev.SWEEP_HUDSON), (g2, dev.SWEEP_REGION), (g1[0], dev.SWEEP_DIVERSITY), (g1[0], dev.SWEEP_SUMMARY))
    if S.window_is_whole(case):
        for g, mode in pairs + ((g2, dev.SWEEP_WC),):
            assert dev.sweep_window(dm, g, mode) == (0, S.window_vectors(case), -1), ("the whole row", mode)
    if S.derives_a_group(case):
        for g, mode in pairs[:3]:
            assert dev.sweep_window(dm, g, mode)[2] >= 0, ("a derived group", mode)
    if not case.has_packed:
        return
    if S.tiled_forced(case):
        for g, mode in pairs:
            assert dev.sweep_tiled(dm, g, mode)[0], ("the tiled route", mode)
    if case.options().get("FMH_TILED") == "0":
        for g, mode in pairs:
            assert not dev.sweep_tiled(dm, g, mode)[0], ("FMH_TILED=0", mode)


@pytest.mark.parametrize("seed", list(range(CASES)) + [s for s in REGRESSION_SEEDS if s >= CASES])
def test_every_call_on_one_matrix(dev, fmh_opts, seed):
    import torch

    case = S.draw(seed)
    for key, value in case.options().items():
        fmh_opts.setenv(key, value)  # FMH_ROW_HI, FMH_COLUMN_WINDOW and FMH_TILED_PLANES are read when the matrix is made
    own = torch.cuda.Stream() if case.own_stream else None
    stream = stream_handle(own)
    dm, x, called, keepalive = S.build(dev, case)
    try:
        assert (dm.variants, dm.samples, dm.ploidy, dm.has_missing, dm.max_allele) == (case.rows, case.samples, case.ploidy, case.missing, case.max_allele)
        if case.layout_at_sweep:
            fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the byte kernels, on a matrix that holds both images
        co = Cohort(case, x, called)
        check_summaries(dev, dm, case, co, stream)
        if case.pair is not None:
            g2 = dev.Groups(dm, case.pair)
            g1 = [dev.Groups(dm, case.pair[p:p + 1]) for p in range(2)]
            off1, off2 = np.nonzero(case.pair[0])[0], np.nonzero(case.pair[1])[0]
            check_probes(dev, dm, g2, g1, case)
            separate = check_hudson_sweeps(dev, dm, g2, case, co, off1, off2, stream)
            check_fused(dev, dm, g2, g1, case, co, off1, off2, separate, stream)
            check_wc_sweeps(dev, dm, case, co, stream)
        check_pairwise(dev, fmh_opts, dm, case, co, stream)
        check_pca_scan(dev, dm, case, co, stream)
        if "pca_gram" in case.runs:
            check_pca_gram(dev, dm, case, co, stream)
        # the matrix itself, after all of them
        data, words = dm.download()
        assert np.array_equal(data.reshape(case.rows, case.columns), co.whole), "download"
        assert (words is None) == (called is None) and (called is None or np.array_equal(words, co.whole_words)), "download: the missing words"
        if case.origin in ("wrap", "wrap-pack"):  # the library never writes wrapped memory
            for buffer, block in zip(keepalive, S.F.wrap_blocks(case)):
                assert np.array_equal(buffer.to_numpy(np.uint8, block.size), block.reshape(-1)), "a wrapped block changed"
    finally:
        dm.close()
        for buffer in keepalive:
            buffer.free()
