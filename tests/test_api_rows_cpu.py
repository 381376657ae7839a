"""The rows and samples every device statistic's Python entry point puts in play, where no row is left: no variant, a region that holds
no row, a Population without a variant.  None of these paths touches a device, so the file runs where there is no GPU.  Pinned for every
entry point and its Population twin: the result (every array: dtype, shape, values) or the refusal (type and exact message), and which
refusal comes FIRST when two arguments are wrong at once - the order differs between the families and is part of the surface."""

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fm():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    import ferromic

    return ferromic


def records(n_sites=4, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, 0] for s in range(n_samples)]) for i in range(n_sites)]


V = records()
NO_ROW = (1000, 2000)   # a well-formed region beyond every position
BAD_REGION = (30, 20)   # end < start
HAPS = [(0, 0), (0, 1), (2, 0)]  # sample 0 whole, sample 2 by its left side only
Y3, CASES3, W4 = np.array([0.0, 1.0, 0.5]), np.array([0.0, 1.0, 0.0]), np.ones(4)

FIELDS = {
    "GenotypeQC": "samples kept_rows hom_ref het hom_alt call_rate alt_frequency maf f_is hwe_p sample_hom_ref sample_het sample_hom_alt "
                  "sample_weighted_called sample_call_rate sample_het_rate sample_f",
    "Kinship": "samples sites both het_het ibs0 het_hom kinship ibs_distance",
    "AssociationScan": "beta se t p n_called alt_frequency positions df covariates_kept covariates_dropped",
    "LogisticScan": "score variance chi2 z p beta se n_called alt_frequency positions n_cases fitted iterations reason covariates_kept covariates_dropped",
    "PolygenicScore": "score average n_called dosage_sum rows_used exponents positions mode",
    "HaplotypeWindows": "sample_size windows sum_squares distinct top_counts h1 h12 h123 h2_h1 haplotype_diversity first_identical",
    "HaplotypeScan": "sample_size focal_rows core_counts area2 pair_steps steps flags ihh sl ihs nsl pairs",
    "SiteFrequencySpectrum": "counts sample_size multiallelic_sites incomplete_sites segregating_sites theta_pi theta_w theta_h tajimas_d fay_wu_h",
}


def arr(dtype, shape, values):
    return (dtype, tuple(shape), repr(values))


def snap(result):
    """Every public field of a result: arrays as (dtype, shape, repr of the values) - repr so that a NaN equals a NaN - scalars as repr."""
    def one(v):
        return arr(str(v.dtype), v.shape, v.tolist()) if isinstance(v, np.ndarray) else repr(v)

    if isinstance(result, np.ndarray):
        return one(result)
    return {k: one(getattr(result, k)) for k in FIELDS[type(result).__name__].split()}


nan = float("nan")


def qc_without_rows(samples):
    n = len(samples)
    out = {k: arr("float64", (0,), []) for k in ("call_rate", "alt_frequency", "maf", "f_is", "hwe_p")}
    out.update({k: arr("uint32", (0,), []) for k in ("hom_ref", "het", "hom_alt")})
    out.update({k: arr("uint64", (n,), [0] * n) for k in ("sample_hom_ref", "sample_het", "sample_hom_alt", "sample_weighted_called")})
    out.update({k: arr("float64", (n,), [nan] * n) for k in ("sample_call_rate", "sample_het_rate", "sample_f")})
    out.update(samples=arr("int64", (n,), samples), kept_rows="0")
    return out


def kinship_without_rows(samples):
    n = len(samples)
    out = {k: arr("uint64", (n, n), [[0] * n] * n) for k in ("both", "het_het", "ibs0", "het_hom")}
    out.update({k: arr("float64", (n, n), [[nan] * n] * n) for k in ("kinship", "ibs_distance")})
    out.update(samples=arr("int64", (n,), samples), sites=arr("int64", (0,), []))
    return out


def scan_without_rows(tables, extra):
    out = {k: arr("float64", (0, 1), []) for k in tables}
    out.update(n_called=arr("uint32", (0,), []), alt_frequency=arr("float64", (0,), []), positions=arr("int64", (0,), []),
               covariates_kept=arr("int64", (0,), []), covariates_dropped=arr("int64", (0,), []))
    out.update(extra)
    return out


ASSOC_WITHOUT_ROWS = scan_without_rows(("beta", "se", "t", "p"), dict(df="1"))
LOGISTIC_WITHOUT_ROWS = scan_without_rows(("score", "variance", "chi2", "z", "p", "beta", "se"),
                                          dict(n_cases=arr("uint64", (1,), [1]), fitted=arr("bool", (1,), [True]),
                                               iterations=arr("int32", (1,), [1]), reason=arr("int32", (1,), [0])))


def score_without_rows(n):
    return dict(score=arr("float64", (n, 1), [[0.0]] * n), average=arr("float64", (n, 1), [[nan]] * n), n_called=arr("uint64", (n,), [0] * n),
                dosage_sum=arr("uint64", (n,), [0] * n), rows_used="0", exponents=arr("int32", (1,), [0]), positions=arr("int64", (0,), []),
                mode="'mean'")


# one window that holds no row: one class of everyone
GARUD_WITHOUT_ROWS = dict(sample_size="3", windows=arr("uint64", (1, 2), [[0, 0]]), sum_squares=arr("uint64", (1,), [9]),
                          distinct=arr("uint32", (1,), [1]), top_counts=arr("uint32", (1, 3), [[3, 0, 0]]), h1=arr("float64", (1,), [1.0]),
                          h12=arr("float64", (1,), [1.0]), h123=arr("float64", (1,), [1.0]), h2_h1=arr("float64", (1,), [0.0]),
                          haplotype_diversity=arr("float64", (1,), [0.0]), first_identical="None")
EHH_WITHOUT_ROWS = dict(sample_size="3", focal_rows=arr("uint64", (0,), []), core_counts=arr("uint32", (0, 2), []),
                        area2=arr("uint64", (0, 2, 2), []), pair_steps=arr("uint64", (0, 2, 2), []), steps=arr("uint32", (0, 2, 2), []),
                        flags=arr("uint32", (0, 2), []), ihh=arr("float64", (0, 2), []), sl=arr("float64", (0, 2), []),
                        ihs=arr("float64", (0,), []), nsl=arr("float64", (0,), []), pairs="None")
SFS_WITHOUT_ROWS = dict(counts=arr("uint64", (4,), [0, 0, 0, 0]), sample_size="3", multiallelic_sites="0", incomplete_sites="0",
                        segregating_sites="0", theta_pi="0.0", theta_w="0.0", theta_h="0.0", tajimas_d="nan", fay_wu_h="0.0")
SFS_WINDOW_WITHOUT_ROWS = dict(counts=arr("uint64", (1, 4), [[0, 0, 0, 0]]), sample_size="3", multiallelic_sites=arr("uint64", (1,), [0]),
                               incomplete_sites=arr("uint64", (1,), [0]), segregating_sites=arr("uint64", (1,), [0]),
                               theta_pi=arr("float64", (1,), [0.0]), theta_w=arr("float64", (1,), [0.0]), theta_h=arr("float64", (1,), [0.0]),
                               tajimas_d=arr("float64", (1,), [nan]), fay_wu_h=arr("float64", (1,), [0.0]))
LD_R2_WITHOUT_ROWS = arr("float64", (0, 3), [])
LD_PRUNE_WITHOUT_ROWS = arr("bool", (0,), [])


def refused(message, call):
    with pytest.raises(ValueError) as caught:
        call()
    assert str(caught.value) == message, (str(caught.value), message)


def haplotype_family(fm, variants, region):
    """The haplotype statistics and LD over a variant list that leaves no row in play: sample_size is len(haplotypes) on [] (no mask),
    the members on a region without a row (all three are columns here)."""
    assert snap(fm.garud_h(variants, HAPS, region=region)) == GARUD_WITHOUT_ROWS
    assert snap(fm.ehh_scan(variants, HAPS, region=region)) == EHH_WITHOUT_ROWS
    assert snap(fm.ihs(variants, HAPS, region=region)) == EHH_WITHOUT_ROWS
    assert snap(fm.nsl(variants, HAPS, region=region)) == EHH_WITHOUT_ROWS
    assert snap(fm.site_frequency_spectrum(variants, HAPS, region=region)) == SFS_WITHOUT_ROWS
    assert snap(fm.site_frequency_spectrum(variants, HAPS, region=region, windows=[(0, 5)])) == SFS_WINDOW_WITHOUT_ROWS
    assert snap(fm.ld_r2(variants, HAPS, 3, region=region)) == LD_R2_WITHOUT_ROWS
    assert snap(fm.ld_prune(variants, HAPS, 3, 0.5, region=region)) == LD_PRUNE_WITHOUT_ROWS


def test_no_variant(fm):
    """[] has no sample either: the cohort statistics refuse the empty sample list, each in its own words; the haplotype family answers."""
    refused("at least one sample is required for genotype QC", lambda: fm.genotype_qc([]))
    refused("at least one sample is required for kinship", lambda: fm.kinship([]))
    refused("at least one sample is required for an association scan", lambda: fm.association_scan([], np.zeros(0)))
    refused("at least one sample is required for a logistic scan", lambda: fm.logistic_scan([], np.zeros(0)))
    refused("at least one sample is required for a polygenic score", lambda: fm.polygenic_score([], np.zeros(0)))
    for call in (lambda: fm.genotype_qc([], samples=[0]), lambda: fm.kinship([], samples=[0]), lambda: fm.association_scan([], Y3, samples=[0]),
                 lambda: fm.logistic_scan([], CASES3, samples=[0]), lambda: fm.polygenic_score([], np.zeros(0), samples=[0])):
        refused("sample 0 is outside the variants' 0 samples", call)
    haplotype_family(fm, [], None)
    # a haplotype that is no column of anything still counts on []: there is no mask to look it up in
    assert fm.garud_h([], [(99, 0)]).sample_size == 1 and fm.site_frequency_spectrum([], [(99, 0)]).sample_size == 1
    assert fm.ehh_scan([], [(99, 0)]).sample_size == 1


def test_region_without_a_row(fm):
    assert snap(fm.genotype_qc(V, region=NO_ROW)) == qc_without_rows([0, 1, 2])
    assert snap(fm.genotype_qc(V, samples=[0, 2], region=NO_ROW)) == qc_without_rows([0, 2])
    assert snap(fm.kinship(V, region=NO_ROW)) == kinship_without_rows([0, 1, 2])
    assert snap(fm.association_scan(V, Y3, region=NO_ROW)) == ASSOC_WITHOUT_ROWS
    assert snap(fm.logistic_scan(V, CASES3, region=NO_ROW)) == LOGISTIC_WITHOUT_ROWS
    assert snap(fm.polygenic_score(V, np.zeros(0), region=NO_ROW)) == score_without_rows(3)
    assert snap(fm.polygenic_score(V, np.zeros(0), samples=[1], region=NO_ROW)) == score_without_rows(1)
    haplotype_family(fm, V, NO_ROW)
    # a sites mask is checked against the rows in play (none), the weights likewise
    refused("sites has 4 entries for 0 rows", lambda: fm.genotype_qc(V, sites=np.ones(4, dtype=bool), region=NO_ROW))
    refused("sites has 4 entries for 0 rows", lambda: fm.kinship(V, sites=np.ones(4, dtype=bool), region=NO_ROW))
    refused("weights has 4 rows, expected one per row in play (0)", lambda: fm.polygenic_score(V, W4, region=NO_ROW))
    # once a store exists the members are looked up: LD does not refuse a haplotype list none of which is a column, the others do
    assert snap(fm.ld_r2(V, [(9, 0), (8, 0)], 3, region=NO_ROW)) == LD_R2_WITHOUT_ROWS
    for call in (lambda: fm.garud_h(V, [(9, 0)], region=NO_ROW), lambda: fm.ehh_scan(V, [(9, 0)], region=NO_ROW),
                 lambda: fm.site_frequency_spectrum(V, [(9, 0)], region=NO_ROW)):
        refused("none of the haplotypes is a column of the variants", call)


def empty_populations(fm):
    store = fm.Population("p", [], HAPS, 100)
    dense = fm.Population.from_numpy("p", np.zeros((0, 3, 2), dtype=np.int8), np.zeros(0, dtype=np.int64), HAPS, 100)
    return store, dense


def test_population_without_a_variant(fm):
    """A store population without a variant has no sample; a dense one keeps its array's sample axis, so sample 0 (both sides listed)
    is in play and sample 2 (one side) is not."""
    store, dense = empty_populations(fm)
    refused("at least one sample is required for genotype QC", store.genotype_qc)
    refused("at least one sample is required for kinship", store.kinship)
    refused("at least one sample is required for an association scan", lambda: store.association_scan(np.zeros(0)))
    refused("at least one sample is required for a logistic scan", lambda: store.logistic_scan(np.zeros(0)))
    refused("at least one sample with both haplotypes in the population is required for a polygenic score",
            lambda: store.polygenic_score(np.zeros(0)))
    assert snap(dense.genotype_qc()) == qc_without_rows([0])
    assert snap(dense.kinship()) == kinship_without_rows([0])
    assert snap(dense.polygenic_score(np.zeros(0))) == score_without_rows(1)
    refused("phenotypes has 0 rows, expected one per selected sample (1)", lambda: dense.association_scan(np.zeros(0)))
    refused("phenotypes has 0 rows, expected one per selected sample (1)", lambda: dense.logistic_scan(np.zeros(0)))
    refused("sites has 2 entries for 0 rows", lambda: dense.genotype_qc(sites=np.ones(2, dtype=bool)))
    for pop in (store, dense):
        assert snap(pop.garud_h()) == GARUD_WITHOUT_ROWS
        assert snap(pop.ehh_scan()) == EHH_WITHOUT_ROWS
        assert snap(pop.ihs()) == EHH_WITHOUT_ROWS
        assert snap(pop.nsl()) == EHH_WITHOUT_ROWS
        assert snap(pop.site_frequency_spectrum()) == SFS_WITHOUT_ROWS
        assert snap(pop.site_frequency_spectrum(windows=[(0, 5)])) == SFS_WINDOW_WITHOUT_ROWS
        assert snap(pop.ld_r2(3)) == LD_R2_WITHOUT_ROWS
        assert snap(pop.ld_prune(3, 0.5)) == LD_PRUNE_WITHOUT_ROWS
    for make in (lambda h: fm.Population("q", [], h, 100), lambda h: dense.with_haplotypes("q", h)):
        refused("at least one haplotype is required for haplotype homozygosity", make([]).garud_h)
        refused("at least one haplotype is required for haplotype homozygosity", make([]).ehh_scan)
        refused("at least one haplotype is required for a site frequency spectrum", make([]).site_frequency_spectrum)
        refused("at least two haplotypes are required for linkage disequilibrium", lambda: make([(0, 0)]).ld_r2(3))


REGION_MESSAGE = "region end must be greater than or equal to region start"

# (what is wrong, the call, the refusal that comes first)
FIRST_REFUSALS = [
    # bad samples + bad region: the sample list is read before the region, everywhere
    ("genotype_qc: samples, region", lambda fm: fm.genotype_qc(V, samples=[2, 1], region=BAD_REGION), "samples must be strictly ascending"),
    ("kinship: samples, region", lambda fm: fm.kinship(V, samples=[7], region=BAD_REGION), "sample 7 is outside the variants' 3 samples"),
    ("association_scan: samples, region", lambda fm: fm.association_scan(V, Y3, samples=[1, 1], region=BAD_REGION), "samples must be strictly ascending"),
    ("logistic_scan: samples, region", lambda fm: fm.logistic_scan(V, CASES3, samples=[-1], region=BAD_REGION), "sample -1 is outside the variants' 3 samples"),
    ("polygenic_score: samples, region", lambda fm: fm.polygenic_score(V, W4, samples=[9], region=BAD_REGION), "sample 9 is outside the variants' 3 samples"),
    # an empty sample list is no bad sample list: genotype_qc and kinship read the region first and refuse it later (after `sites`)
    ("genotype_qc: no sample, region", lambda fm: fm.genotype_qc(V, samples=[], region=BAD_REGION), REGION_MESSAGE),
    ("kinship: no sample, region", lambda fm: fm.kinship(V, samples=[], region=BAD_REGION), REGION_MESSAGE),
    ("genotype_qc: no sample, sites", lambda fm: fm.genotype_qc(V, samples=[], sites=np.ones(4, dtype=bool), region=NO_ROW),
     "at least one sample is required for genotype QC"),
    # bad model + bad region: the scans fit the model, which needs len(samples), before they read the region
    ("association_scan: model, region", lambda fm: fm.association_scan(V, np.zeros(2), region=BAD_REGION),
     "phenotypes has 2 rows, expected one per selected sample (3)"),
    ("association_scan: samples, model", lambda fm: fm.association_scan(V, np.zeros(2), samples=[2, 1]), "samples must be strictly ascending"),
    ("association_scan: no sample, region", lambda fm: fm.association_scan(V, np.zeros(0), samples=[], region=BAD_REGION),
     "at least one sample is required for an association scan"),
    ("logistic_scan: model, region", lambda fm: fm.logistic_scan(V, np.zeros((3, 0)), region=BAD_REGION), "at least one phenotype is required"),
    ("logistic_scan: no sample, region", lambda fm: fm.logistic_scan(V, np.zeros(0), samples=[], region=BAD_REGION),
     "at least one sample is required for a logistic scan"),
    # bad weights + empty samples: the score reads the region, then the weights against the rows in play, then refuses the empty list
    ("polygenic_score: weights, no sample", lambda fm: fm.polygenic_score(V, np.ones(3), samples=[]),
     "weights has 3 rows, expected one per row in play (4)"),
    ("polygenic_score: region, weights, no sample", lambda fm: fm.polygenic_score(V, np.ones(3), samples=[], region=BAD_REGION), REGION_MESSAGE),
    ("polygenic_score: no sample", lambda fm: fm.polygenic_score(V, W4, samples=[]), "at least one sample is required for a polygenic score"),
    ("polygenic_score: mode, samples", lambda fm: fm.polygenic_score(V, W4, samples=[9], missing="none"), 'missing must be "mean" or "zero", got "none"'),
    # on [] the cohort statistics never read the region
    ("genotype_qc: [], region", lambda fm: fm.genotype_qc([], region=BAD_REGION), "at least one sample is required for genotype QC"),
    ("polygenic_score: [], region", lambda fm: fm.polygenic_score([], np.zeros(0), region=BAD_REGION), "at least one sample is required for a polygenic score"),
    # empty haplotypes + bad region: emptiness first, then the region, and only then the variants
    ("garud_h: no haplotype, region", lambda fm: fm.garud_h(V, [], region=BAD_REGION), "at least one haplotype is required for haplotype homozygosity"),
    ("ehh_scan: no haplotype, region", lambda fm: fm.ehh_scan(V, [], region=BAD_REGION), "at least one haplotype is required for haplotype homozygosity"),
    ("ihs: no haplotype, region", lambda fm: fm.ihs(V, [], region=BAD_REGION), "at least one haplotype is required for haplotype homozygosity"),
    ("nsl: no haplotype, region", lambda fm: fm.nsl(V, [], region=BAD_REGION), "at least one haplotype is required for haplotype homozygosity"),
    ("site_frequency_spectrum: no haplotype, region", lambda fm: fm.site_frequency_spectrum(V, [], region=BAD_REGION),
     "at least one haplotype is required for a site frequency spectrum"),
    ("ld_r2: one haplotype, region", lambda fm: fm.ld_r2(V, [(0, 0)], 3, region=BAD_REGION), "at least two haplotypes are required for linkage disequilibrium"),
    ("ld_prune: no haplotype, region", lambda fm: fm.ld_prune(V, [], 3, 0.5, region=BAD_REGION), "at least two haplotypes are required for linkage disequilibrium"),
    ("garud_h: region, variants", lambda fm: fm.garud_h([dict(nothing=1)], HAPS, region=BAD_REGION), REGION_MESSAGE),
    ("garud_h: region, []", lambda fm: fm.garud_h([], HAPS, region=BAD_REGION), REGION_MESSAGE),
    ("ehh_scan: region, []", lambda fm: fm.ehh_scan([], HAPS, region=BAD_REGION), REGION_MESSAGE),
    ("site_frequency_spectrum: region, []", lambda fm: fm.site_frequency_spectrum([], HAPS, region=BAD_REGION), REGION_MESSAGE),
    ("garud_h: region, members", lambda fm: fm.garud_h(V, [(9, 0)], region=BAD_REGION), REGION_MESSAGE),
    ("garud_h: windows, region", lambda fm: fm.garud_h(V, HAPS, region=BAD_REGION, step=2), "step needs size"),
    ("ld_r2: region", lambda fm: fm.ld_r2(V, HAPS, 3, region=BAD_REGION), REGION_MESSAGE),
    ("ld_prune: region", lambda fm: fm.ld_prune(V, HAPS, 3, 0.5, region=BAD_REGION), REGION_MESSAGE),
]


@pytest.mark.parametrize("what, call, message", FIRST_REFUSALS, ids=[row[0] for row in FIRST_REFUSALS])
def test_first_refusal(fm, what, call, message):
    refused(message, lambda: call(fm))


def test_ld_reads_the_region_only_when_there_is_a_variant(fm):
    """Unlike the haplotype windows, LD parses `region` after the variants, and not at all on []."""
    assert snap(fm.ld_r2([], HAPS, 3, region=BAD_REGION)) == LD_R2_WITHOUT_ROWS
    assert snap(fm.ld_prune([], HAPS, 3, 0.5, region=BAD_REGION)) == LD_PRUNE_WITHOUT_ROWS
