"""The rows and samples the Python entry points put in play, on the device: for each of the ten statistics (a) a region equals the slice
of the variant list it selects, (b) a Population equals the variant list with the samples both of whose haplotypes it holds, (c) the same
for a from_numpy (dense) Population - every result array bitwise (dtype, shape, values; NaN equal to NaN).

One 60-row, 12-sample diploid record list with missing genotypes (test_gpu_qc.py::test_genotype_qc_of_variant_records's): the smallest
that has a region cutting rows off both ends, a sample with one haplotype listed, a sample index beyond the cohort, and both a store and a
dense Population."""

import numpy as np
import pytest

from tests.test_api_rows_cpu import snap
from tests.test_gpu_sfs import cohort

pytestmark = pytest.mark.gpu

ROWS, SAMPLES = 60, 12
REGION, CUT = (155, 612), slice(6, 52)  # positions 160 .. 610: rows 6 .. 51
BOTH = [0, 1, 3, 4, 6, 7, 9, 10, 11]
HAPS = [(s, side) for s in BOTH for side in (0, 1)] + [(5, 0), (SAMPLES, 0), (SAMPLES, 1)]  # sample 5 by its left side, sample 12 is nobody


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


@pytest.fixture(scope="module")
def data():
    x, called = cohort(ROWS, 2 * SAMPLES, 1, True, seed=24)
    whole = np.repeat(called[:, 0::2], 2, axis=1)  # a record's genotype is missing as a whole
    assert not whole.all() and whole[CUT].any(axis=1).all()
    positions = 100 + 10 * np.arange(ROWS, dtype=np.int64)
    variants = [dict(position=int(positions[i]), genotypes=[None if not whole[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])]
                                                            for s in range(SAMPLES)]) for i in range(ROWS)]
    geno = np.where(whole, x, -1).astype(np.int8).reshape(ROWS, SAMPLES, 2)
    rng = np.random.default_rng(5)
    return dict(variants=variants, geno=geno, positions=positions, y=rng.normal(size=SAMPLES), cov=rng.normal(size=(SAMPLES, 1)),
                cases=(np.arange(SAMPLES) % 3 == 0).astype(np.float64), weights=rng.normal(size=(ROWS, 2)))


@pytest.fixture(scope="module")
def populations(fm, data):
    return [fm.Population("p", data["variants"], HAPS, 1000), fm.Population.from_numpy("p", data["geno"], data["positions"], HAPS, 1000)]


# name -> (over a variant list: f(fm, variants, rows, samples, region), over a Population: f(pop)); `rows` cuts the per-row argument
def cohort_statistics(d):
    y, cov, cases, w = d["y"], d["cov"], d["cases"], d["weights"]
    pick = lambda a, samples: a if samples is None else a[samples]
    return {
        "genotype_qc": (lambda fm, v, rows, samples, region: fm.genotype_qc(v, samples=samples, region=region), lambda pop: pop.genotype_qc()),
        "kinship": (lambda fm, v, rows, samples, region: fm.kinship(v, samples=samples, region=region), lambda pop: pop.kinship()),
        "association_scan": (lambda fm, v, rows, samples, region: fm.association_scan(v, pick(y, samples), pick(cov, samples), samples=samples, region=region),
                             lambda pop: pop.association_scan(y[BOTH], cov[BOTH])),
        "logistic_scan": (lambda fm, v, rows, samples, region: fm.logistic_scan(v, pick(cases, samples), samples=samples, region=region),
                          lambda pop: pop.logistic_scan(cases[BOTH])),
        "polygenic_score": (lambda fm, v, rows, samples, region: fm.polygenic_score(v, w[rows], samples=samples, region=region),
                            lambda pop: pop.polygenic_score(w)),
    }


# name -> (f(fm, variants, region), f(pop)); the haplotypes are HAPS on both sides
HAPLOTYPE_STATISTICS = {
    "garud_h": (lambda fm, v, region: fm.garud_h(v, HAPS, region=region, size=7, step=3, partition=True), lambda pop: pop.garud_h(size=7, step=3, partition=True)),
    "ehh_scan": (lambda fm, v, region: fm.ehh_scan(v, HAPS, region=region, max_extent=9, curve=True), lambda pop: pop.ehh_scan(max_extent=9, curve=True)),
    "ihs": (lambda fm, v, region: fm.ihs(v, HAPS, region=region), lambda pop: pop.ihs()),
    "nsl": (lambda fm, v, region: fm.nsl(v, HAPS, region=region), lambda pop: pop.nsl()),
    "site_frequency_spectrum": (lambda fm, v, region: fm.site_frequency_spectrum(v, HAPS, region=region, windows=[(0, 300), (250, 10000)]),
                                lambda pop: pop.site_frequency_spectrum(windows=[(0, 300), (250, 10000)])),
    "ld_r2": (lambda fm, v, region: fm.ld_r2(v, HAPS, 5, region=region), lambda pop: pop.ld_r2(5)),
    "ld_prune": (lambda fm, v, region: fm.ld_prune(v, HAPS, 8, 0.3, region=region), lambda pop: pop.ld_prune(8, 0.3)),
}


def something_in(result):
    """The comparison is not between two empty results."""
    s = snap(result)
    shapes = [s[1]] if isinstance(s, tuple) else [v[1] for k, v in s.items() if isinstance(v, tuple) and not k.startswith("covariates_")]
    assert shapes and all(0 not in shape for shape in shapes), s
    return s


@pytest.mark.parametrize("name", ["genotype_qc", "kinship", "association_scan", "logistic_scan", "polygenic_score"])
def test_cohort_statistic(fm, data, populations, name):
    over_variants, over_population = cohort_statistics(data)[name]
    v = data["variants"]
    assert something_in(over_variants(fm, v, CUT, None, REGION)) == snap(over_variants(fm, v[CUT], CUT, None, None)), "(a) region == slice"
    listed = something_in(over_variants(fm, v, slice(None), BOTH, None))
    assert listed != snap(over_variants(fm, v, slice(None), None, None)), "the sample list matters"
    for pop, kind in zip(populations, ("(b) store", "(c) dense")):
        assert snap(over_population(pop)) == listed, kind


@pytest.mark.parametrize("name", list(HAPLOTYPE_STATISTICS))
def test_haplotype_statistic(fm, data, populations, name):
    over_variants, over_population = HAPLOTYPE_STATISTICS[name]
    v = data["variants"]
    assert something_in(over_variants(fm, v, REGION)) == snap(over_variants(fm, v[CUT], None)), "(a) region == slice"
    listed = something_in(over_variants(fm, v, None))
    for pop, kind in zip(populations, ("(b) store", "(c) dense")):
        assert snap(over_population(pop)) == listed, kind
