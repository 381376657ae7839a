"""Crossing fuzz of the nine cohort statistics - LD, the spectra, haplotype windows, EHH scans, f-statistic moments, kinship counts,
genotype QC counts, association sums and hom-alt sums - against their oracles in tests/*_ref.py.

One test per seed (tests/cohort_fuzz.py draws the case; tests/test_cohort_fuzz_draws_cpu.py shows what the default seeds cover): the matrix
is made ONCE, through one of the library's six ways of making one - fmh_matrix_create, fmh_matrix_create_packed at the device's pitch and
at a foreign one, fmh_matrix_wrap + fmh_matrix_pack of caller-owned rows whose padding is junk, fmh_matrix_generate + fmh_matrix_pack, and a
second generation on an already packed matrix - and every statistic the ploidy allows runs on that same matrix, one after another, with
crossed arguments: a sample list, a row range with both ends off 16, a keep mask, row tables on / off / default, a small grid, short
items and a stream of the case's own.  So no call may leave state behind for the next, and the matrix comes out of all of them unchanged.

Each result is compared exactly as in that statistic's own file: array_equal on the integer tables, the same bits on r^2 (NaN positions
equal), `over` words with zero padding bits, outputs pre-filled with 0xA5 where the wrapper offers it.  Two checks need no oracle: the
download after the statistics is the cohort with zeros under the missing entries, and fmh_genotype_counts agrees with fmh_assoc_sums of a
column of ones.

FERROMIC_FUZZ_COHORT_CASES sets the number of seeds (default 48)."""

import os

import numpy as np
import pytest

from tests import assoc_ref, cohort_fuzz as F, ehh_ref, fstat_ref, hap_ref, kinship_ref, ld_ref, logistic_ref, qc_ref, sfs_ref
from tests.helpers import assert_bits_equal

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("FERROMIC_FUZZ_COHORT_CASES", str(F.DEFAULT_CASES)))
# seeds that once failed, with the cause
REGRESSION_SEEDS = [
    9,  # fmh_matrix_download of a wrapped matrix copied the caller's byte rows as they were: junk under the missing entries, where the header promises 0
]
EHH_FIELDS = ("area2", "pair_steps", "steps", "core", "flags", "reserved")
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


def rows_of(a, case):
    return None if a is None else a[case.row_begin : case.row_begin + case.row_count]


def check_ld(dev, dm, x, called, case, stream):
    mask = F.ld_column_mask(case)
    g = None if mask is None else dev.Groups(dm, mask[None, :].astype(np.uint8))
    try:
        got = dev.ld_band(dm, g, case.band, F.LD_THRESHOLD, case.row_begin, case.row_count, stream=stream)
        keep = dev.ld_prune(dm, g, case.band, F.LD_THRESHOLD, case.row_begin, case.row_count, chunk_rows=case.prune_chunk, stream=stream)
    finally:
        if g is not None:
            g.close()
    ref = ld_ref.band(x, called, mask, case.row_begin, case.row_count, case.row_begin + case.row_count, case.band, F.LD_THRESHOLD)
    for key in ("n_ab", "n_joint", "site_n", "site_alt"):
        assert np.array_equal(getattr(got, key), ref[key]), ("ld", key)
    assert_bits_equal(got.r2.reshape(-1), ref["r2"].reshape(-1), "ld r2")
    assert got.over.shape == ref["over"].shape and np.array_equal(got.over, ref["over"]), ("ld", "over")
    if case.band % 32:
        assert not (got.over[:, -1] >> np.uint32(case.band % 32)).any(), "the padding bits of the last word are zero"
    assert np.array_equal(keep, ld_ref.greedy_from_r2(ref["r2"], F.LD_THRESHOLD)), "ld_prune"


def check_sfs(dev, dm, x, called, case, stream):
    g = dev.Groups(dm, case.half[None, :].astype(np.uint8))
    try:
        got = dev.sfs(dm, g, case.windows, stream=stream)
    finally:
        g.close()
    counts, multi, incomplete = sfs_ref.sfs(x, called, case.half, case.windows)
    assert got.counts.dtype == np.uint64 and got.counts.shape == counts.shape and np.array_equal(got.counts, counts), "sfs"
    assert np.array_equal(got.multiallelic, multi) and np.array_equal(got.incomplete, incomplete), "sfs tallies"


def check_sfs_joint(dev, dm, x, called, case, stream):
    g = dev.Groups(dm, case.pair.astype(np.uint8))
    try:
        got = dev.sfs_joint(dm, g, case.row_begin, case.row_count, stream=stream)
    finally:
        g.close()
    ref = sfs_ref.sfs_joint(x, called, case.pair[0], case.pair[1], case.row_begin, case.row_count)
    assert np.array_equal(got.counts, ref[0]) and (got.multiallelic, got.incomplete) == ref[1:], "sfs_joint"


def check_haplotype_windows(dev, dm, x, called, case, stream):
    g = dev.Groups(dm, case.half[None, :].astype(np.uint8))
    try:
        got = dev.haplotype_windows(dm, g, case.windows, partition=True, stream=stream, fill=FILL)
    finally:
        g.close()
    ref = hap_ref.windows(x, called, case.half, case.windows)
    assert got.sum_sq.dtype == np.uint64 and got.distinct.dtype == np.uint32 and got.top.dtype == np.uint32 and got.first.dtype == np.uint32
    for key in ("sum_sq", "distinct", "top", "first"):
        assert np.array_equal(getattr(got, key), ref[key]), ("haplotype_windows", key)


def check_ehh(dev, dm, x, called, case, stream):
    kw = dict(row_begin=case.row_begin, row_end=case.row_begin + case.row_count, min_ehh=(1, 20), max_extent=25, curve=True)
    g = dev.Groups(dm, case.half[None, :].astype(np.uint8))
    try:
        got = dev.ehh_scan(dm, g, case.focal, stream=stream, fill=FILL, **kw)
    finally:
        g.close()
    sides, pairs = ehh_ref.scan(x, called, case.half, case.focal, **kw)
    assert got.sides.shape == sides.shape
    for name in EHH_FIELDS:
        assert np.array_equal(got.sides[name], sides[name]), ("ehh", name)
    assert got.pairs.dtype == np.uint32 and np.array_equal(got.pairs, pairs), ("ehh", "pairs")


def check_fstat(dev, dm, x, called, case, stream):
    got = dev.fstat_moments(dm, case.groups.astype(np.uint8), case.windows, stream=stream)
    table, multi, incomplete = fstat_ref.moments(x, called, case.groups, case.windows)
    assert got.moments.dtype == np.uint64 and got.moments.shape == table.shape and np.array_equal(got.moments, table), "fstat"
    assert np.array_equal(got.multiallelic, multi) and np.array_equal(got.incomplete, incomplete), "fstat tallies"


def check_kinship(dev, dm, x, called, case, stream):
    samples, n_samples = F.sample_arguments(case.kin_sel, case.kin_prefix)
    got = dev.kinship_counts(dm, samples=samples, n_samples=n_samples, row_begin=case.row_begin, row_count=case.row_count, keep=case.keep, stream=stream)
    ref = kinship_ref.tables(rows_of(x, case), rows_of(called, case), case.kin_sel, case.keep)
    for name, r in zip(dev.KINSHIP_TABLES, ref):
        t = getattr(got, name)
        assert t.dtype == np.uint64 and t.shape == r.shape and np.array_equal(t, r), ("kinship", name)
    assert got.kept_rows == (case.row_count if case.keep is None else int(np.count_nonzero(case.keep)))


def check_qc(dev, dm, x, called, case, stream):
    samples, n_samples = F.sample_arguments(case.sel, case.as_prefix)
    got = dev.genotype_counts(dm, samples=samples, n_samples=n_samples, row_begin=case.row_begin, row_count=case.row_count, keep=case.keep, stream=stream,
                              fill=FILL)
    xs, cs = rows_of(x, case), rows_of(called, case)
    for name, ref in zip(dev.QC_CLASSES, qc_ref.site_tracks(xs, cs, case.sel)):
        t = got.site[name]
        assert t.dtype == np.uint32 and t.shape == ref.shape and np.array_equal(t, ref), ("qc site", name)
    for name, ref in zip(dev.QC_CLASSES, qc_ref.sample_tables(xs, cs, case.sel, case.keep)):
        t = got.sample[name]
        assert t.dtype == np.uint64 and t.shape == ref.shape and np.array_equal(t, ref), ("qc sample", name)
    assert got.kept_rows == (case.row_count if case.keep is None else int(np.count_nonzero(case.keep)))


def check_assoc_and_homalt(dev, dm, x, called, case, stream):
    samples, n_samples = F.sample_arguments(case.sel, case.as_prefix)
    values = F.values(case)
    xs, cs = rows_of(x, case), rows_of(called, case)
    got = dev.assoc_sums(dm, values, samples=samples, n_samples=n_samples, row_begin=case.row_begin, row_count=case.row_count, stream=stream, fill=FILL)
    S, Cs = assoc_ref.sums(xs, cs, values, case.sel)
    assert got.dosage.dtype == np.int64 and got.dosage.shape == S.shape and np.array_equal(got.dosage, S), "assoc S"
    assert np.array_equal(got.called, Cs), "assoc C"
    hom = dev.assoc_homalt_sums(dm, values, samples=samples, n_samples=n_samples, row_begin=case.row_begin, row_count=case.row_count, stream=stream, fill=FILL)
    ref = logistic_ref.homalt_sums(xs, cs, values, case.sel)
    assert hom.dtype == np.int64 and hom.shape == ref.shape and np.array_equal(hom, ref), "homalt"


def check_counts_against_sums_of_ones(dev, dm, case, stream):
    """Two device paths that need no oracle: the class counts of every row over all samples, and the sums of a column of ones."""
    counts = dev.genotype_counts(dm, sample=(), stream=stream, fill=FILL).site
    ones = dev.assoc_sums(dm, np.ones((case.samples, 1), dtype=np.int32), stream=stream, fill=FILL)
    hom_ref, het, hom_alt = (counts[name].astype(np.int64) for name in dev.QC_CLASSES)
    assert np.array_equal(ones.dosage[:, 0], het + 2 * hom_alt) and np.array_equal(ones.called[:, 0], hom_ref + het + hom_alt)


@pytest.mark.parametrize("seed", list(range(CASES)) + [s for s in REGRESSION_SEEDS if s >= CASES])
def test_every_statistic_on_one_matrix(dev, fmh_opts, seed):
    import torch

    case = F.draw(seed)
    for key, value in case.options().items():
        fmh_opts.setenv(key, value)  # FMH_ROW_HI is read when the matrix is made
    own = torch.cuda.Stream() if case.own_stream else None
    stream = F.stream_handle(own)
    assert (stream is not None and bool(stream.value)) == case.own_stream, "a stream of its own, not the NULL stream"
    dm, x, called, keepalive = F.build(dev, case)
    try:
        assert (dm.variants, dm.samples, dm.ploidy, dm.has_missing) == (case.rows, case.samples, case.ploidy, case.missing)
        if case.origin not in F.HOST_ORIGINS:  # the device's generator against its twin in numpy
            ref_x, ref_called = F.generated(case)
            assert np.array_equal(x, ref_x) and (called is None) == (ref_called is None) and (called is None or np.array_equal(called, ref_called))
        check_ld(dev, dm, x, called, case, stream)
        check_sfs(dev, dm, x, called, case, stream)
        if "sfs_joint" in case.runs:
            check_sfs_joint(dev, dm, x, called, case, stream)
        check_haplotype_windows(dev, dm, x, called, case, stream)
        check_ehh(dev, dm, x, called, case, stream)
        if "fstat" in case.runs:
            check_fstat(dev, dm, x, called, case, stream)
        if case.ploidy == 2:
            check_kinship(dev, dm, x, called, case, stream)
            check_qc(dev, dm, x, called, case, stream)
            check_assoc_and_homalt(dev, dm, x, called, case, stream)
            check_counts_against_sums_of_ones(dev, dm, case, stream)
        # the matrix itself, after all of them: the cohort, with zeros under the missing entries whichever route made it
        data, words = dm.download()
        expected = x if called is None else np.where(called, x, 0).astype(np.uint8)
        assert np.array_equal(data.reshape(case.rows, case.columns), expected), "download"
        assert (words is None) == (called is None)
        if called is not None:
            assert np.array_equal(words, F.missing_words(called)), "download: the missing words"
    finally:
        dm.close()
        for buffer in keepalive:
            buffer.free()
