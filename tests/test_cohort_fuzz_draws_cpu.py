"""The draws of tests/test_gpu_cohort_fuzz.py, replayed without a device: the default seeds do cross what the fuzz claims to cross, and the
junk its inputs carry would show in the counts of a library that read it.  Conditions on the inputs only - nothing here weighs a result."""

import itertools

import numpy as np
import pytest

from tests import cohort_fuzz as F
from tests.test_gpu_sfs import KINDS


@pytest.fixture(scope="module")
def cases():
    return [F.draw(seed) for seed in range(F.DEFAULT_CASES)]


def runs(cases, *statistics):
    return [c for c in cases if any(s in c.runs for s in statistics)]


def test_a_case_is_its_seed_alone(cases):
    for case in cases[:6]:
        again = F.draw(case.seed)
        for name, value in vars(case).items():
            other = getattr(again, name)
            assert np.array_equal(value, other) if isinstance(value, np.ndarray) else value == other, name


def test_origins_kinds_and_row_tables_are_crossed(cases):
    for origin, kind in itertools.product(F.ORIGINS, KINDS):
        assert sum(c.origin == origin and c.kind == kind for c in cases) >= 2, (origin, kind)
    for origin, row_hi in itertools.product(F.ORIGINS, F.ROW_HI):
        assert any(c.origin == origin and c.row_hi == row_hi for c in cases), (origin, row_hi)
    for ploidy in (1, 2, 3):
        assert sum(c.ploidy == ploidy for c in cases) >= 6, ploidy
    assert {c.release_bytes for c in cases if c.origin == "generate-pack"} == {False, True}
    for case in cases:
        assert set(F.COLUMN_STATISTICS) - {"sfs_joint", "fstat"} <= set(case.runs)
        assert (case.ploidy == 2) == all(s in case.runs for s in F.DIPLOID_STATISTICS)
        assert (case.ploidy == 2) or not any(s in case.runs for s in F.DIPLOID_STATISTICS)


def test_foreign_pitches_meet_ragged_rows(cases):
    for origin in ("wrap-pack", "planes-pitch"):
        mine = [c for c in cases if c.origin == origin]
        assert sum(c.columns % 128 != 0 for c in mine) >= 3, origin
        assert any(c.columns % 8 != 0 for c in mine), origin
    for case in cases:
        row_bytes = (case.columns + 7) // 8
        if case.origin == "planes-pitch":
            planes, called_plane, pitch = F.plane_arrays(case)
            assert pitch == row_bytes + case.extra and pitch != F.round_up(row_bytes, 16), "a pitch the device does not use"
            x, called = F.truth(case)
            for plane in planes + ([] if called_plane is None else [called_plane]):
                assert (plane[:, row_bytes:] == 0xFF).all()
                bits = np.unpackbits(plane[:, :row_bytes], axis=1, bitorder="little")
                assert not bits[:, case.columns:].any(), "the bits past the last column inside the row's last byte are zero"
            if called_plane is not None:
                assert np.array_equal(np.unpackbits(called_plane[:, :row_bytes], axis=1, bitorder="little")[:, : case.columns].astype(bool), called)
        if case.origin == "wrap-pack":
            assert case.pitch % 16 == 0 and case.pitch >= case.columns
            assert case.bits_pitch % 4 == 0 and case.bits_pitch * 8 >= F.round_up(case.columns, 16)


def test_a_foreign_pitch_is_never_the_devices_own():
    """At the device's pitch the header wants zero padding bytes, and the 0xFF this fuzz puts there would be counted: 125 + 3 = 128 bytes at
    1 000 columns (seed 326 of a longer walk).  Every seed a longer walk may reach, draws only."""
    for seed in range(2, 3000, 6):
        case = F.draw(seed)
        row_bytes = (case.columns + 7) // 8
        assert case.origin == "planes-pitch" and row_bytes + case.extra != F.round_up(row_bytes, 16), seed


def test_the_junk_of_a_wrapped_matrix_would_show(cases):
    """A pack that did not mask the padding, or an allele-overflow check that looked at it, is visible on every wrap-pack case."""
    seen_rows = seen_bits = 0
    for case in (c for c in cases if c.origin == "wrap-pack"):
        x, called = F.truth(case)
        H = case.columns
        block, bits = F.wrap_blocks(case)
        plane0, called_plane = F.unmasked_planes(case)
        everyone = np.ones(x.shape, dtype=bool) if called is None else called
        assert np.array_equal(block[:, :H][everyone], x[everyone]), "the called entries are the cohort's"
        assert x[everyone].max(initial=0) <= case.max_allele
        himask = 0xFF & ~((1 << (1 if case.max_allele <= 1 else 2 if case.max_allele <= 3 else 3)) - 1)
        if case.pitch > H:
            seen_rows += 1
            spread = np.unpackbits(plane0, axis=1, bitorder="little")
            assert spread[:, H:].any(), "a set bit past the last column in plane 0"
            assert (spread.sum(axis=1) != spread[:, :H].sum(axis=1)).any(), "and row popcounts that differ from the masked plane's"
            assert (block[:, H:] & himask).any(), "a padding byte with bits above max_allele"
        if called is not None:
            assert (block[:, :H][~called] & himask).any(), "a byte under an uncalled entry with bits above max_allele"
        if called_plane is not None and case.bits_pitch * 8 > H:
            seen_bits += 1
            spread = np.unpackbits(called_plane, axis=1, bitorder="little")
            assert np.array_equal(spread[:, :H].astype(bool), called)
            assert spread[:, H:].any(), "a set called-bit past the last column"
            assert (spread.sum(axis=1) != called.sum(axis=1)).any(), "a row whose popcount is not its called count"
    assert seen_rows >= 3 and seen_bits >= 2


def test_a_regenerated_matrix_needs_its_row_table_rebuilt(cases):
    seen = 0
    for case in (c for c in cases if c.origin == "regenerate"):
        _, first_called = F.host_generate(case.rows, case.columns, *F.generator_arguments(case, first=True))
        assert first_called.all(), "the first generation leaves every row clean"
        x, called = F.generated(case)
        assert x.max() <= 1 and (called is None) == (not case.missing)
        if case.missing:
            seen += 1
            full = called.all(axis=1)
            assert full.any() and not full.all(), "a fully called row and a row with an uncalled entry"
            assert not x[~called].any(), "the byte of a missing entry is zero"
    assert seen >= 4


def test_every_argument_shape_occurs_where_its_statistic_runs(cases):
    diploid = runs(cases, *F.DIPLOID_STATISTICS)
    for shape in F.SAMPLE_LISTS:
        assert sum(c.sample_list == shape for c in diploid) >= 2, shape
    for shape in F.ROW_RANGES:
        assert sum(c.row_range == shape for c in diploid) >= 2 and sum(c.row_range == shape for c in cases) >= 2, shape
    for shape in F.KEEP_MASKS:
        assert sum(c.keep_mask == shape for c in runs(cases, "kinship", "qc")) >= 2, shape
    for shape in F.LD_MASKS:
        assert sum(c.ld_mask == shape for c in runs(cases, "ld")) >= 2, shape
    for k in F.VALUE_COLUMNS:
        assert sum(c.value_columns == k for c in diploid) >= 2, k
    for band in F.LD_BANDS:
        assert sum(c.band == band for c in cases) >= 2, band
    for name, values in (("grid_blocks", F.GRID_BLOCKS), ("item_rows", F.ITEM_ROWS), ("own_stream", (False, True))):
        for value in values:
            assert sum(getattr(c, name) == value for c in cases) >= 2, (name, value)
    assert sum(c.kin_sel is not c.sel for c in diploid) >= 1, "a matrix too wide for the kinship oracle gets a prefix or a shorter list"
    for case in cases:
        H, rows = case.columns, case.rows
        if case.row_range == "inside":
            assert case.row_begin % 16 and (case.row_begin + case.row_count) % 16 and 0 < case.row_begin and case.row_begin + case.row_count <= rows
        else:
            assert (case.row_begin, case.row_count) == (0, rows)
        assert case.keep is None or case.keep.shape == (case.row_count,)
        if case.sel is not None:
            assert (np.diff(case.sel) > 0).all() and case.sel[-1] < case.samples and (not case.as_prefix or case.sel.size < case.samples)
        if case.kin_sel is not None:
            assert case.kin_sel.size <= F.KINSHIP_MAX_SAMPLES and (np.diff(case.kin_sel) > 0).all() and case.kin_sel[-1] < case.samples
        else:
            assert case.samples <= F.KINSHIP_MAX_SAMPLES
        assert case.half.shape == (H,) and case.half.any()
        if case.confined is not None:
            assert case.confined.any() and not case.confined[:384].any() and not case.confined[768:].any()
        assert (case.ld_mask == "confined") <= (case.confined is not None)
        for partition, lo, hi in ((case.pair, 2, 2), (case.groups, 2, 9)):
            if partition is not None:
                assert lo <= partition.shape[0] <= hi and (partition.sum(axis=0) == 1).all() and partition.any(axis=1).all()
        assert (case.pair is None) == (H < 2) and (case.groups is None) == (H < 2)
        assert sum(b == e for b, e in case.windows) >= 1 and any(e == rows and b < e for b, e in case.windows)
        assert all(0 <= b <= e <= rows for b, e in case.windows)
        assert all(case.row_begin <= f < case.row_begin + case.row_count for f in case.focal)


def test_the_crossing_no_other_test_has(cases):
    """A sample list, a row range, non-default item rows and a stream of the case's own, all on one call."""
    crossed = [c for c in runs(cases, *F.DIPLOID_STATISTICS)
               if c.sample_list != "none" and c.row_range == "inside" and c.item_rows is not None and c.own_stream]
    assert len(crossed) >= 4, [c.seed for c in crossed]
