"""ferromic.ibd_segments, Population.ibd_segments and IbdSegments where no device is needed (as tests/test_roh_api_cpu.py does for the runs
of homozygosity): the summaries IbdSegments.from_segments builds on the host, the coverage track, the IBD fraction, the segment order of
fmh_ibd_sort_segments behind it, the result (every array: dtype, shape, values) for a region without a row, a sites mask that keeps no
row, a single sample and a Population without a variant, and which refusal comes FIRST when two arguments are wrong at once -
runs_of_homozygosity's order, with the scan's own parameters read before anything else."""

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("samples mode n_segments total_sites total_length longest kept_rows segment_a segment_b segment_first_row segment_last_row "
          "segment_start segment_end segment_sites segment_missing").split()


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


def without_segments(samples, kept_rows=0, mode="ibd1"):
    n = len(samples)
    out = {k: arr("uint64", (n, n), [[0] * n] * n) for k in ("n_segments", "total_sites", "total_length", "longest")}
    out.update({k: arr("uint32", (0,), []) for k in ("segment_a", "segment_b", "segment_sites", "segment_missing")})
    out.update({k: arr("uint64", (0,), []) for k in ("segment_first_row", "segment_last_row")})
    out.update({k: arr("int64", (0,), []) for k in ("segment_start", "segment_end")})
    out.update(samples=arr("int64", (n,), samples), kept_rows=str(kept_rows), mode=repr(mode))
    return out


def refused(message, call, kind=ValueError):
    with pytest.raises(kind) as caught:
        call()
    assert str(caught.value) == message, (str(caught.value), message)


def test_names_are_exported(fm):
    assert fm.IbdSegments.__module__.endswith("_core") and callable(fm.ibd_segments) and hasattr(fm.Population, "ibd_segments")


def test_region_without_a_row(fm):
    r = fm.ibd_segments(V, region=NO_ROW)
    assert snap(r) == without_segments([0, 1, 2])
    assert repr(r) == "IbdSegments(mode=ibd1, samples=3, kept_rows=0, segments=0)" and len(r) == 3
    assert r.ibd_fraction().shape == (3, 3) and np.isnan(r.ibd_fraction()).all()           # NaN without rows
    assert r.ibd_fraction(genome_length=1000).tolist() == [[0.0] * 3] * 3
    assert arr(str(r.site_coverage().dtype), r.site_coverage().shape, r.site_coverage().tolist()) == arr("uint32", (0,), [])
    assert snap(fm.ibd_segments(V, samples=[0, 2], region=NO_ROW, mode="ibd2")) == without_segments([0, 2], mode="ibd2")
    p = r.params
    assert p == dict(mode="ibd1", min_sites=436, min_length=7_000_000, max_gap=1_000_000, max_bp_per_site=None, max_missing=None)   # IBIS's defaults
    no_segments = fm.ibd_segments(V, region=NO_ROW, segments=False)
    assert no_segments.n_segments.tolist() == [[0] * 3] * 3
    refused("the result holds no segments: it was computed with segments=False", lambda: no_segments.segment_a)
    refused("the result holds no segments: it was computed with segments=False", no_segments.site_coverage)
    refused("sites has 4 entries for 0 rows", lambda: fm.ibd_segments(V, sites=np.ones(4, dtype=bool), region=NO_ROW))


def test_one_sample_and_no_kept_row_need_no_device(fm):
    """One sample has no pair and a sites mask may keep no row: both are answered on the host (this test runs where there is no device)."""
    one = fm.ibd_segments(V, samples=[1])
    assert snap(one) == without_segments([1], kept_rows=4)
    assert one.ibd_fraction().tolist() == [[0.0]] and one.site_coverage().tolist() == [0, 0, 0, 0]
    assert repr(one) == "IbdSegments(mode=ibd1, samples=1, kept_rows=4, segments=0)" and len(one) == 1
    none = fm.ibd_segments(V, sites=np.zeros(4, dtype=bool), mode="ibd2")
    assert snap(none) == without_segments([0, 1, 2], mode="ibd2")
    assert np.isnan(none.ibd_fraction()).all() and none.site_coverage().tolist() == [0, 0, 0, 0]
    pop = fm.Population.from_numpy("p", np.zeros((4, 3, 2), dtype=np.int8), np.arange(4) * 10, HAPS, 100)
    assert snap(pop.ibd_segments()) == without_segments([0], kept_rows=4)           # only sample 0 is whole
    # the positions are still checked
    down = [dict(position=p, genotypes=[[0, 0], [0, 0]]) for p in (10, 30, 20)]
    refused("the positions descend at variant 2: IBD segments need them in order", lambda: fm.ibd_segments(down, samples=[0]))


def test_population_without_a_variant(fm):
    store = fm.Population("p", [], HAPS, 100)
    dense = fm.Population.from_numpy("p", np.zeros((0, 3, 2), dtype=np.int8), np.zeros(0, dtype=np.int64), HAPS, 100)
    refused("at least one sample with both haplotypes in the population is required for IBD segments", store.ibd_segments)
    assert snap(dense.ibd_segments()) == without_segments([0])
    refused("sites has 2 entries for 0 rows", lambda: dense.ibd_segments(sites=np.ones(2, dtype=bool)))
    refused("at least one sample is required for IBD segments", lambda: fm.ibd_segments([]))
    refused("sample 0 is outside the variants' 0 samples", lambda: fm.ibd_segments([], samples=[0]))


FIRST_REFUSALS = [
    # runs_of_homozygosity's order: the sample list, then the region, then the empty list, then `sites`
    ("samples, region", lambda fm: fm.ibd_segments(V, samples=[2, 1], region=BAD_REGION), "samples must be strictly ascending"),
    ("sample range, region", lambda fm: fm.ibd_segments(V, samples=[7], region=BAD_REGION), "sample 7 is outside the variants' 3 samples"),
    ("no sample, region", lambda fm: fm.ibd_segments(V, samples=[], region=BAD_REGION), REGION_MESSAGE),
    ("no sample, sites", lambda fm: fm.ibd_segments(V, samples=[], sites=np.ones(4, dtype=bool), region=NO_ROW),
     "at least one sample is required for IBD segments"),
    ("[], region", lambda fm: fm.ibd_segments([], region=BAD_REGION), "at least one sample is required for IBD segments"),
    ("sites, one sample", lambda fm: fm.ibd_segments(V, samples=[1], sites=np.ones(3, dtype=bool)), "sites has 3 entries for 4 rows"),
    # the scan's own parameters are read before the variants
    ("mode, samples", lambda fm: fm.ibd_segments(V, samples=[9], mode="ibd3"), 'mode must be "ibd1" or "ibd2", got "ibd3"'),
    ("mode, region", lambda fm: fm.ibd_segments(V, region=BAD_REGION, mode=""), 'mode must be "ibd1" or "ibd2", got ""'),
    ("mode, min_sites", lambda fm: fm.ibd_segments(V, mode="IBD1", min_sites=-1), 'mode must be "ibd1" or "ibd2", got "IBD1"'),
    ("min_sites, samples", lambda fm: fm.ibd_segments(V, samples=[9], min_sites=-1), "min_sites must be within 0 .. 2^32 - 1"),
    ("min_length, max_gap", lambda fm: fm.ibd_segments(V, min_length=1 << 32, max_gap=-5), "min_length must be within 0 .. 2^32 - 1"),
    ("max_gap", lambda fm: fm.ibd_segments(V, max_gap=-5), "max_gap must be within 0 .. 2^32 - 2 or None"),
    ("max_missing, region", lambda fm: fm.ibd_segments(V, region=BAD_REGION, max_missing=0xFFFFFFFF), "max_missing must be within 0 .. 2^32 - 2 or None"),
    ("haploid", lambda fm: fm.ibd_segments([dict(position=1, genotypes=[[0], [1]])]), "IBD segments take diploid genotypes (ploidy 2), got ploidy 1"),
]


@pytest.mark.parametrize("what, call, message", FIRST_REFUSALS, ids=[row[0] for row in FIRST_REFUSALS])
def test_first_refusal(fm, what, call, message):
    refused(message, lambda: call(fm))


def test_from_segments_builds_the_summaries(fm):
    """Three samples (numbers 2, 5, 7), eight rows at positions 0, 100, .., 700, four segments handed over out of order: the pair (0, 1)
    holds rows 4..6 and 0..1, the pair (0, 2) rows 0..2, the pair (1, 2) rows 5..7.  length = position(last) - position(first) + 1."""
    h = fm.IbdSegments.from_segments(samples=[2, 5, 7], segment_a=[0, 1, 0, 0], segment_b=[1, 2, 2, 1], segment_first_row=[4, 5, 0, 0],
                                     segment_last_row=[6, 7, 2, 1], segment_sites=[3, 3, 3, 2], segment_missing=[0, 2, 0, 1], positions=np.arange(8) * 100)
    assert snap(h) == dict(
        samples=arr("int64", (3,), [2, 5, 7]), mode=repr("ibd1"),
        n_segments=arr("uint64", (3, 3), [[0, 2, 1], [2, 0, 1], [1, 1, 0]]), total_sites=arr("uint64", (3, 3), [[0, 5, 3], [5, 0, 3], [3, 3, 0]]),
        total_length=arr("uint64", (3, 3), [[0, 302, 201], [302, 0, 201], [201, 201, 0]]),
        longest=arr("uint64", (3, 3), [[0, 201, 201], [201, 0, 201], [201, 201, 0]]), kept_rows="8",
        # sorted by (a, b, first_row), as fmh_ibd_sort_segments orders them
        segment_a=arr("uint32", (4,), [0, 0, 0, 1]), segment_b=arr("uint32", (4,), [1, 1, 2, 2]),
        segment_first_row=arr("uint64", (4,), [0, 4, 0, 5]), segment_last_row=arr("uint64", (4,), [1, 6, 2, 7]),
        segment_start=arr("int64", (4,), [0, 400, 0, 500]), segment_end=arr("int64", (4,), [100, 600, 200, 700]),
        segment_sites=arr("uint32", (4,), [2, 3, 3, 3]), segment_missing=arr("uint32", (4,), [1, 0, 0, 2]))
    cover = h.site_coverage()
    assert arr(str(cover.dtype), cover.shape, cover.tolist()) == arr("uint32", (8,), [2, 2, 1, 0, 1, 2, 2, 1])
    assert h.ibd_fraction().tolist() == [[0.0, 302 / 701, 201 / 701], [302 / 701, 0.0, 201 / 701], [201 / 701, 201 / 701, 0.0]]   # 700 - 0 + 1
    assert h.ibd_fraction(genome_length=1000)[0].tolist() == [0.0, 0.302, 0.201]
    assert repr(h) == "IbdSegments(mode=ibd1, samples=3, kept_rows=8, segments=4)" and h.params is None and len(h) == 3
    # a sites mask narrows the kept rows and the default length: rows 1..5 kept -> 500 - 100 + 1
    kept = fm.IbdSegments.from_segments([2, 3], [0], [1], [1], [3], [3], [0], np.arange(8) * 100, sites=np.array([0, 1, 1, 1, 1, 1, 0, 0], dtype=bool),
                                        mode="ibd2")
    assert kept.kept_rows == 5 and kept.ibd_fraction().tolist() == [[0.0, 201 / 401], [201 / 401, 0.0]] and kept.mode == "ibd2"
    empty = fm.IbdSegments.from_segments([4, 9], [], [], [], [], [], [], [])
    assert empty.n_segments.tolist() == [[0, 0], [0, 0]] and np.isnan(empty.ibd_fraction()).all() and empty.site_coverage().shape == (0,)


def test_from_segments_refusals(fm):
    pos = np.arange(4) * 10
    make = fm.IbdSegments.from_segments
    refused("segment_last_row has 1 entries, expected 2", lambda: make([0, 1], [0, 0], [1, 1], [0, 2], [1], [2, 2], [0, 0], pos))
    refused("segment 0 names the pair (0, 2) of 2 samples: a < b < n is required", lambda: make([0, 1], [0], [2], [0], [1], [2], [0], pos))
    refused("segment 0 names the pair (1, 1) of 2 samples: a < b < n is required", lambda: make([0, 1], [1], [1], [0], [1], [2], [0], pos))
    refused("segment 0 names the pair (1, 0) of 2 samples: a < b < n is required", lambda: make([0, 1], [1], [0], [0], [1], [2], [0], pos))
    refused("segment 0 lies outside the 4 rows", lambda: make([0, 1], [0], [1], [2], [4], [3], [0], pos))
    refused("segment 0 lies outside the 4 rows", lambda: make([0, 1], [0], [1], [2], [1], [3], [0], pos))
    refused("the positions descend at row 2", lambda: make([0], [], [], [], [], [], [], [0, 5, 4]))
    refused("genome_length must be positive", lambda: make([0], [], [], [], [], [], [], pos).ibd_fraction(0))
    refused('mode must be "ibd1" or "ibd2", got "x"', lambda: make([0], [], [], [], [], [], [], pos, mode="x"))
