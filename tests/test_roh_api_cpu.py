"""ferromic.runs_of_homozygosity, Population.runs_of_homozygosity and HomozygosityRuns where no row is left or no device is needed (as
tests/test_api_rows_cpu.py does for the other statistics): the summaries HomozygosityRuns.from_segments builds on the host, the coverage
track, F_ROH, the segment order of fmh_roh_sort_segments behind it, the result (every array: dtype, shape, values) for a region without a
row and a Population without a variant, and which refusal comes FIRST when two arguments are wrong at once - genotype_qc's order, with the
scan's own parameters read before anything else."""

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("samples n_runs total_sites total_length longest bin_runs bin_length kept_rows segment_sample segment_first_row segment_last_row "
          "segment_start segment_end segment_sites segment_het segment_missing").split()


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
NO_ROW = (1000, 2000)
BAD_REGION = (30, 20)
HAPS = [(0, 0), (0, 1), (2, 0)]  # sample 0 whole, sample 2 by its left side only
REGION_MESSAGE = "region end must be greater than or equal to region start"


def arr(dtype, shape, values):
    return (dtype, tuple(shape), repr(values))


def snap(result):
    def one(v):
        return arr(str(v.dtype), v.shape, v.tolist()) if isinstance(v, np.ndarray) else repr(v)

    return {k: one(getattr(result, k)) for k in FIELDS}


def without_rows(samples, n_bins=0):
    n = len(samples)
    out = {k: arr("uint64", (n,), [0] * n) for k in ("n_runs", "total_sites", "total_length", "longest")}
    out.update({k: arr("uint64", (n, n_bins), [[0] * n_bins] * n) for k in ("bin_runs", "bin_length")})
    out.update({k: arr("uint32", (0,), []) for k in ("segment_sample", "segment_sites", "segment_het", "segment_missing")})
    out.update({k: arr("uint64", (0,), []) for k in ("segment_first_row", "segment_last_row")})
    out.update({k: arr("int64", (0,), []) for k in ("segment_start", "segment_end")})
    out.update(samples=arr("int64", (n,), samples), kept_rows="0")
    return out


def refused(message, call, kind=ValueError):
    with pytest.raises(kind) as caught:
        call()
    assert str(caught.value) == message, (str(caught.value), message)


def test_names_are_exported(fm):
    assert fm.HomozygosityRuns.__module__.endswith("_core") and callable(fm.runs_of_homozygosity) and hasattr(fm.Population, "runs_of_homozygosity")


def test_region_without_a_row(fm):
    r = fm.runs_of_homozygosity(V, region=NO_ROW)
    assert snap(r) == without_rows([0, 1, 2])
    assert repr(r) == "HomozygosityRuns(samples=3, kept_rows=0, runs=0)" and len(r) == 3
    assert r.f_roh().tolist() != r.f_roh().tolist() and np.isnan(r.f_roh()).all()          # NaN without rows
    assert r.f_roh(genome_length=1000).tolist() == [0.0, 0.0, 0.0]
    assert arr(str(r.site_coverage().dtype), r.site_coverage().shape, r.site_coverage().tolist()) == arr("uint32", (0,), [])
    assert snap(fm.runs_of_homozygosity(V, samples=[0, 2], region=NO_ROW, length_bins=[10, 20])) == without_rows([0, 2], n_bins=3)
    p = r.params
    assert p["window"] == 50 and p["window_het"] == 1 and p["window_missing"] == 5 and p["window_threshold"] == 0.05       # PLINK's defaults
    assert p["min_sites"] == 100 and p["min_length"] == 1_000_000 and p["max_gap"] == 1_000_000 and p["max_bp_per_site"] == 50_000
    assert p["max_het"] is None and p["max_missing"] is None and p["length_bins"] is None
    assert p["need"][1] == 1 and p["need"][20] == 1 and p["need"][21] == 2 and p["need"][50] == 3 and len(p["need"]) == 51
    no_segments = fm.runs_of_homozygosity(V, region=NO_ROW, segments=False)
    assert no_segments.n_runs.tolist() == [0, 0, 0]
    refused("the result holds no segments: it was computed with segments=False", lambda: no_segments.segment_sample)
    refused("the result holds no segments: it was computed with segments=False", no_segments.site_coverage)
    refused("sites has 4 entries for 0 rows", lambda: fm.runs_of_homozygosity(V, sites=np.ones(4, dtype=bool), region=NO_ROW))


def test_population_without_a_variant(fm):
    store = fm.Population("p", [], HAPS, 100)
    dense = fm.Population.from_numpy("p", np.zeros((0, 3, 2), dtype=np.int8), np.zeros(0, dtype=np.int64), HAPS, 100)
    refused("at least one sample with both haplotypes in the population is required for runs of homozygosity", store.runs_of_homozygosity)
    assert snap(dense.runs_of_homozygosity()) == without_rows([0])
    refused("sites has 2 entries for 0 rows", lambda: dense.runs_of_homozygosity(sites=np.ones(2, dtype=bool)))
    refused("at least one sample is required for runs of homozygosity", lambda: fm.runs_of_homozygosity([]))
    refused("sample 0 is outside the variants' 0 samples", lambda: fm.runs_of_homozygosity([], samples=[0]))


FIRST_REFUSALS = [
    # genotype_qc's order: the sample list, then the region, then the empty list, then `sites`
    ("samples, region", lambda fm: fm.runs_of_homozygosity(V, samples=[2, 1], region=BAD_REGION), "samples must be strictly ascending"),
    ("sample range, region", lambda fm: fm.runs_of_homozygosity(V, samples=[7], region=BAD_REGION), "sample 7 is outside the variants' 3 samples"),
    ("no sample, region", lambda fm: fm.runs_of_homozygosity(V, samples=[], region=BAD_REGION), REGION_MESSAGE),
    ("no sample, sites", lambda fm: fm.runs_of_homozygosity(V, samples=[], sites=np.ones(4, dtype=bool), region=NO_ROW),
     "at least one sample is required for runs of homozygosity"),
    ("[], region", lambda fm: fm.runs_of_homozygosity([], region=BAD_REGION), "at least one sample is required for runs of homozygosity"),
    # the scan's own parameters are read before the variants
    ("window, samples", lambda fm: fm.runs_of_homozygosity(V, samples=[9], window=65), "window must be within 1 .. 64, got 65"),
    ("window, region", lambda fm: fm.runs_of_homozygosity(V, region=BAD_REGION, window=0), "window must be within 1 .. 64, got 0"),
    ("threshold, samples", lambda fm: fm.runs_of_homozygosity(V, samples=[9], window_threshold=1.5), "window_threshold must be within 0 .. 1"),
    ("window, threshold", lambda fm: fm.runs_of_homozygosity(V, window=99, window_threshold=-1.0), "window must be within 1 .. 64, got 99"),
    ("bins, samples", lambda fm: fm.runs_of_homozygosity(V, samples=[9], length_bins=[5, 5]), "length_bins must be strictly ascending"),
    ("too many bins", lambda fm: fm.runs_of_homozygosity(V, length_bins=list(range(1, 9))), "8 length bin edges: at most 7 (8 bins) are taken"),
    ("min_sites, bins", lambda fm: fm.runs_of_homozygosity(V, min_sites=-1, length_bins=[5, 5]), "min_sites must be within 0 .. 2^32 - 1"),
    ("max_gap", lambda fm: fm.runs_of_homozygosity(V, max_gap=-5), "max_gap must be within 0 .. 2^32 - 2 or None"),
]


@pytest.mark.parametrize("what, call, message", FIRST_REFUSALS, ids=[row[0] for row in FIRST_REFUSALS])
def test_first_refusal(fm, what, call, message):
    refused(message, lambda: call(fm))


def test_from_segments_builds_the_summaries(fm):
    """Three samples (numbers 2, 5, 7), eight rows at positions 0, 100, .., 700, three segments handed over out of order: entry 1 holds rows
    4..6 and 0..1, entry 0 rows 0..2.  length = position(last) - position(first) + 1; edges (150, 250): 101 -> bin 0, 201 -> bin 1."""
    h = fm.HomozygosityRuns.from_segments(samples=[2, 5, 7], segment_sample=[1, 0, 1], segment_first_row=[4, 0, 0], segment_last_row=[6, 2, 1],
                                          segment_sites=[3, 3, 2], segment_het=[0, 1, 0], segment_missing=[0, 0, 1], positions=np.arange(8) * 100,
                                          length_bins=[150, 250])
    assert snap(h) == dict(
        samples=arr("int64", (3,), [2, 5, 7]), n_runs=arr("uint64", (3,), [1, 2, 0]), total_sites=arr("uint64", (3,), [3, 5, 0]),
        total_length=arr("uint64", (3,), [201, 302, 0]), longest=arr("uint64", (3,), [201, 201, 0]),
        bin_runs=arr("uint64", (3, 3), [[0, 1, 0], [1, 1, 0], [0, 0, 0]]), bin_length=arr("uint64", (3, 3), [[0, 201, 0], [101, 201, 0], [0, 0, 0]]),
        kept_rows="8",
        # sorted by (sample, first_row), as fmh_roh_sort_segments orders them
        segment_sample=arr("uint32", (3,), [0, 1, 1]), segment_first_row=arr("uint64", (3,), [0, 0, 4]), segment_last_row=arr("uint64", (3,), [2, 1, 6]),
        segment_start=arr("int64", (3,), [0, 0, 400]), segment_end=arr("int64", (3,), [200, 100, 600]),
        segment_sites=arr("uint32", (3,), [3, 2, 3]), segment_het=arr("uint32", (3,), [1, 0, 0]), segment_missing=arr("uint32", (3,), [0, 1, 0]))
    cover = h.site_coverage()
    assert arr(str(cover.dtype), cover.shape, cover.tolist()) == arr("uint32", (8,), [2, 2, 1, 0, 1, 1, 1, 0])
    assert h.f_roh().tolist() == [201 / 701, 302 / 701, 0.0]                  # the default length: 700 - 0 + 1
    assert h.f_roh(genome_length=1000).tolist() == [0.201, 0.302, 0.0]
    assert repr(h) == "HomozygosityRuns(samples=3, kept_rows=8, runs=3)" and h.params is None
    # a sites mask narrows the kept rows and the default length: rows 1..5 kept -> 500 - 100 + 1
    kept = fm.HomozygosityRuns.from_segments([2], [0], [1], [3], [3], [0], [0], np.arange(8) * 100, sites=np.array([0, 1, 1, 1, 1, 1, 0, 0], dtype=bool))
    assert kept.kept_rows == 5 and kept.f_roh().tolist() == [201 / 401] and kept.bin_runs.shape == (1, 0)
    empty = fm.HomozygosityRuns.from_segments([4, 9], [], [], [], [], [], [], [])
    assert empty.n_runs.tolist() == [0, 0] and np.isnan(empty.f_roh()).all() and empty.site_coverage().shape == (0,)


def test_from_segments_refusals(fm):
    pos = np.arange(4) * 10
    refused("segment_last_row has 1 entries, expected 2", lambda: fm.HomozygosityRuns.from_segments([0], [0, 0], [0, 2], [1], [2, 2], [0, 0], [0, 0], pos))
    refused("segment 0 names entry 1 of 1 samples", lambda: fm.HomozygosityRuns.from_segments([0], [1], [0], [1], [2], [0], [0], pos))
    refused("segment 0 lies outside the 4 rows", lambda: fm.HomozygosityRuns.from_segments([0], [0], [2], [4], [3], [0], [0], pos))
    refused("segment 0 lies outside the 4 rows", lambda: fm.HomozygosityRuns.from_segments([0], [0], [2], [1], [3], [0], [0], pos))
    refused("the positions descend at row 2", lambda: fm.HomozygosityRuns.from_segments([0], [], [], [], [], [], [], [0, 5, 4]))
    refused("genome_length must be positive", lambda: fm.HomozygosityRuns.from_segments([0], [], [], [], [], [], [], pos).f_roh(0))
