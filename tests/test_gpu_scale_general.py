"""Full-scale oracle gates for the sweeps real cohorts take besides the biallelic, complete one: multi-allelic rows (the GENERAL kernels,
four- and sixteen-lane rows, two and three planes), sparse and dense row tables (row_hi: rows with a bit above plane 0; row_gap: rows
with an uncalled column) and W&C with five to seven groups (the exact kernels) and with more than eight (the pair-totals kernels).

Every cohort is built on the host - the counter-based biallelic stream of oracle/dense.py, then a seeded set of rows overwritten with
multi-allelic values and / or given missing calls (data 0 under a missing call) - uploaded with DeviceMatrix.from_host under the default
options (at these sizes the row tables are built), and compared with the C oracle on the same bytes: per-site f64 tracks bit for bit,
counts exactly, regional sums to 1e-9."""

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.helpers import build_cohort, thresholds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


def check_hudson(got, exp, general, what):
    for name in ("fst", "dxy", "pi1", "pi2", "num", "den"):
        H.assert_bits_equal(got.sites[name], getattr(exp, name), f"{name} {what}")
    assert np.array_equal(got.sites["called"], exp.called), what
    for p in range(2):
        assert got.pop[p]["segregating_sites"] == exp.pop[p]["segregating_sites"], (p, what)
        assert got.pop[p]["uncallable_sites"] == exp.pop[p]["uncallable_sites"], (p, what)
        assert H.rel_close(got.pop[p]["pi_sum"], exp.pop[p]["pi_sum"]), (p, what)
    if general:
        for k in ("site_num_sum", "site_den_sum", "site_dxy_sum"):
            assert H.rel_close(got.totals[k], exp.totals[k]), (k, what)
        for k in ("sites_with_components", "site_dxy_skipped"):
            assert got.totals[k] == exp.totals[k], (k, what)
    else:
        assert np.array_equal(got.sites["alt"], exp.alt), what
        for k in ("numerator_sum", "denominator_sum", "pi1_sum", "pi2_sum", "dxy_sum_all", "site_num_sum", "site_den_sum"):
            assert H.rel_close(got.totals[k], exp.totals[k]), (k, what)
        for k in ("dxy_uncallable_sites", "sites_with_components"):
            assert got.totals[k] == exp.totals[k], (k, what)


def check_wc(w, exp, what):
    assert np.array_equal(w.state, exp.state), what
    assert np.array_equal(w.a.view(np.uint64), exp.a.view(np.uint64)), what
    assert np.array_equal(w.b.view(np.uint64), exp.b.view(np.uint64)), what
    assert np.array_equal(w.informative_sites, exp.informative), what
    for k in range(len(exp.sum_a)):
        assert H.rel_close(float(w.sum_a[k]), float(exp.sum_a[k])) and H.rel_close(float(w.sum_b[k]), float(exp.sum_b[k])), (k, what)


COHORTS = {
    # rows, samples, multi-allelic fraction, max_allele, gap-row fraction, rebuild without tables
    "A": (1_000_000, 500, 0.002, 3, 0.0, False),    # two planes, sparse row_hi, four-lane rows
    "B": (1_000_000, 500, 0.02, 7, 0.002, True),    # three planes, both tables sparse, GENERAL + MISSING
    "C": (1_000_000, 500, 0.0, 1, 0.002, False),    # biallelic: sparse row_gap, the no-missing core inside a MISSING matrix
    "D": (250_000, 2500, 0.02, 3, 0.005, False),    # sixteen-lane rows
    "E": (200_000, 500, 0.5, 7, 0.0, False),        # row_hi all but full: the dense end
}


@pytest.mark.parametrize("name", list(COHORTS))
def test_cohort_against_c_oracle(dev, fmh_opts, name):
    S, N, frac_multi, max_allele, frac_gap, again = COHORTS[name]
    Hc = 2 * N
    cut = 2 * N // 5
    data, words, multi = build_cohort(S, N, 7919 * (ord(name) - 64), frac_multi, max_allele, frac_gap, cut)
    declared = int(max_allele)
    flat = data.reshape(-1)
    off1, off2 = np.arange(0, 2 * cut), np.arange(2 * cut, Hc - 2)
    masks = np.zeros((2, Hc), dtype=np.uint8)
    masks[0, off1], masks[1, off2] = 1, 1
    exp = D.hudson_sweep_dense(flat, words, S, Hc, declared, off1, off2, 16)
    exp_wc = {}
    goc = {}
    for G in (3, 5):
        goc[G] = np.repeat(np.minimum(np.arange(N) * G // N, G - 1), 2).astype(np.uint8)
        exp_wc[G] = D.wc_sites(flat, words, S, Hc, goc[G], G, 16)
    # population_summaries' alt counts allele 1 on a multi-allelic matrix (the reference builds the summary, whose alt is the sum of the
    # allele values, only for max_allele <= 1): the oracle's gather on every row without an allele above 1, a recount on the others
    exp_alt = exp.alt.copy()
    if len(multi):
        for p, cols in enumerate((off1, off2)):
            sub = data[multi][:, cols] == 1
            if words is not None:
                idx = multi[:, None].astype(np.uint64) * np.uint64(Hc) + cols[None, :].astype(np.uint64)
                sub &= ((words[(idx >> np.uint64(6)).astype(np.int64)] >> (idx & np.uint64(63))) & np.uint64(1)) == 0
            exp_alt[p, multi] = sub.sum(axis=1)

    def run(dm, what):
        assert dm.max_allele == declared
        g2 = dev.Groups(dm, masks)
        check_hudson(dev.hudson_sweep(dm, g2, dev.FORMULA_DENSE), exp, declared > 1, f"Hudson {what}")
        s = dev.population_summaries(dm, g2, dev.FORMULA_DENSE)
        assert np.array_equal(s.called, exp.called), what
        assert np.array_equal(s.alt, exp_alt), what
        for G in (3, 5):
            gg = dev.Groups(dm, np.stack([goc[G] == k for k in range(G)]).astype(np.uint8))
            check_wc(dev.wc_sweep(dm, gg), exp_wc[G], f"W&C {G} groups {what}")

    dm = dev.DeviceMatrix.from_host(flat, words, S, N, 2, declared)
    run(dm, f"cohort {name}")
    dm.close()
    if again:  # the same bytes uploaded without the row tables: the same oracle output
        fmh_opts.setenv("FMH_ROW_HI", "0")
        dm = dev.DeviceMatrix.from_host(flat, words, S, N, 2, declared)
        run(dm, f"cohort {name} without row tables")
        dm.close()
        fmh_opts.delenv("FMH_ROW_HI")
    del data, flat, words, exp, exp_wc


@pytest.fixture(scope="module")
def wc_cohort(dev):
    """1 M sites x 2 000 haplotypes, biallelic, nothing missing: resident packed on the device, regenerated on the host."""
    S, N = 1_000_000, 1000
    seed = 31_337
    thr = thresholds(S, seed)
    poc = np.repeat((np.arange(N) >= N // 2).astype(np.uint8), 2)
    dm = dev.DeviceMatrix.alloc(S, N, 2, with_missing=False)
    dm.generate(seed, 0, thr, poc, 0)
    dm.pack(release_bytes=True)
    hdata, _ = D.generate(S, 2 * N, seed, 0, thr, poc, 0, 16)
    yield dm, hdata, S, N
    dm.close()
    del hdata


def groups_of(N, G, empty=None):
    goc = np.minimum(np.arange(N) * G // N, G - 1)
    if empty is not None:
        goc[goc == empty] = empty + 1  # a group without members takes part in no pair
    return np.repeat(goc, 2).astype(np.uint8)


@pytest.mark.parametrize("G", [5, 6, 7])
def test_wc_exact_group_kernels_full_size(dev, wc_cohort, G):
    """The kernels instantiated for exactly five, six and seven groups over a million sites: every slot's a, b and state at every site bit
    for bit, informative sites exactly, sums to 1e-9."""
    dm, hdata, S, N = wc_cohort
    goc = groups_of(N, G)
    w = dev.wc_sweep(dm, dev.Groups(dm, np.stack([goc == k for k in range(G)]).astype(np.uint8)))
    check_wc(w, D.wc_sites(hdata, None, S, 2 * N, goc, G, 16), f"{G} groups")


@pytest.mark.parametrize("G,empty", [(9, None), (16, 7), (26, None)])
def test_wc_many_groups_totals_full_size(dev, fmh_opts, wc_cohort, G, empty):
    """More than eight groups with no per-site track (the --fst_populations workload: 26 populations): the biallelic pair-totals kernel and
    the general pair kernel (FMH_WC_BI_TOTALS=0) against the oracle's regional sums - informative sites exactly, sums to 1e-9."""
    dm, hdata, S, N = wc_cohort
    goc = groups_of(N, G, empty)
    masks = np.stack([goc == k for k in range(G)]).astype(np.uint8)
    exp = D.wc_sites(hdata, None, S, 2 * N, goc, G, 16, sites=False)
    if empty is not None:
        assert not masks[empty].any()
    for bi_totals in (None, "0"):
        if bi_totals is not None:
            fmh_opts.setenv("FMH_WC_BI_TOTALS", bi_totals)
        got = dev.wc_sweep_many(dm, masks, sites=False)
        what = f"{G} groups, FMH_WC_BI_TOTALS={bi_totals or 'default'}"
        assert np.array_equal(got.informative_sites, exp.informative), what
        for k in range(len(exp.sum_a)):
            assert H.rel_close(float(got.sum_a[k]), float(exp.sum_a[k])), (k, what)
            assert H.rel_close(float(got.sum_b[k]), float(exp.sum_b[k])), (k, what)
    fmh_opts.delenv("FMH_WC_BI_TOTALS")
