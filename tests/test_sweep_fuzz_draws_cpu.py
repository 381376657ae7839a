"""The draws of tests/test_gpu_sweep_fuzz.py, replayed without a device: the default seeds do cross what the fuzz claims to cross.  Conditions
on the inputs only - nothing here weighs a result.  Whether an option is "not a no-op" and which route a sweep takes are judged by
sweep_fuzz.applies and sweep_fuzz.route, the preconditions of ferromic_amd/csrc/sweep_plan.hpp restated on the draw."""

import numpy as np
import pytest

from tests import sweep_fuzz as S

ROUTES = ("tiled", "flat", "mfma", "packed4", "packed16", "packed4_3p", "packed16_3p", "global", "bits", "bytes")


@pytest.fixture(scope="module")
def cases():
    return [S.draw(seed) for seed in range(S.DEFAULT_CASES)]


def test_a_case_is_its_seed_alone(cases):
    for case in cases[:8]:
        again = S.draw(case.seed)
        for name, value in vars(case).items():
            other = getattr(again, name)
            assert np.array_equal(value, other) if isinstance(value, np.ndarray) else value == other, name


def test_origins_meet_kinds_widths_and_row_ranges(cases):
    for origin in S.ORIGINS:
        mine = [c for c in cases if c.origin == origin]
        for kind in set(S.kinds_of(origin)):
            assert sum(c.kind == kind for c in mine) >= 1, (origin, kind)
        for width in S.WIDTHS:
            assert any(c.width == width for c in mine), (origin, width)
        for form in S.ROW_RANGES:
            assert any(c.row_range == form for c in mine), (origin, form)
    assert all(c.max_allele <= 7 for c in cases if c.has_packed), "the planes hold alleles 0..7"
    assert sum(c.max_allele == 9 for c in cases) >= 4
    assert {c.release_bytes for c in cases if c.origin == "generate-pack"} == {False, True}
    for ploidy in (1, 2, 3):
        assert sum(c.ploidy == ploidy for c in cases) >= 12, ploidy


def test_geometry(cases):
    for case in cases:
        H = case.columns
        assert H == case.samples * case.ploidy and S.width_class(H) == case.width
        assert case.samples in S.SAMPLES and case.rows in S.ROWS
        if case.row_range == "inside":
            b, e = case.row_begin, case.row_begin + case.row_count
            assert 0 < b < e <= case.rows and b % 16 and e % 16 and b % 64 and e % 64
        else:
            assert (case.row_begin, case.row_count) == (0, case.rows)
        if case.origin in ("wrap", "wrap-pack"):
            assert case.pitch % 16 == 0 and case.pitch >= H and case.bits_pitch % 4 == 0 and case.bits_pitch * 8 >= S.round_up(H, 16)
        row_bytes = (H + 7) // 8
        assert row_bytes + case.extra != S.round_up(row_bytes, 16), "a foreign pitch is never the device's own"
    # a row range inside one 64-row tile, and one that crosses a tile edge, on a grid of one and of three workgroups
    inside = [c for c in cases if c.row_range == "inside"]
    assert sum(c.row_begin // 64 != (c.row_begin + c.row_count - 1) // 64 for c in inside) >= 8
    for blocks in ("1", "3"):
        assert sum(c.options().get("FMH_GRID_BLOCKS") == blocks for c in inside) >= 6, blocks


def test_groups(cases):
    for geometry in S.GEOMETRIES:
        assert sum(c.geometry == geometry for c in cases) >= 4, geometry
    for case in cases:
        H = case.columns
        assert (case.pair is None) == (H < 2) == (case.wc is None)
        assert case.summary.shape[1] == H and 1 <= case.summary.shape[0] <= 8
        if case.pair is None:
            continue
        G = case.wc.shape[0]
        assert case.pair.shape == (2, H) and 2 <= G <= min(8, H)
        for masks in (case.pair, case.wc):
            assert (masks.sum(axis=0) <= 1).all(), "disjoint"
            covers, empty = (masks.sum(axis=0) == 1).all(), [g for g in range(masks.shape[0]) if not masks[g].any()]
            cols = [np.nonzero(m)[0] for m in masks]
            runs = all(c.size == 0 or c[-1] - c[0] + 1 == c.size for c in cols)
            if case.geometry == "contiguous":
                assert covers and not empty and runs
            elif case.geometry == "hull":
                member = masks.any(axis=0)
                inner = member[np.nonzero(member)[0][0]: np.nonzero(member)[0][-1] + 1]
                assert not member[0] and not member[-1] and (~inner).sum() == 1 and not empty and runs
            elif case.geometry == "confined":
                assert not masks[:, :384].any() and not masks[:, 768:].any() and not empty and H > 384
            elif case.geometry == "empty-group":
                assert len(empty) == 1
            else:
                assert covers and not empty
        assert np.array_equal(case.summary, case.wc) or case.geometry == "overlap"
    overlap = [c for c in cases if c.geometry == "overlap"]
    assert sum(bool((c.summary.sum(axis=0) > 1).any()) for c in overlap) >= 3 and len({c.summary.shape[0] for c in overlap}) >= 3


def test_every_forcing_value_meets_a_matrix_it_acts_on(cases):
    keys = dict(S.OPTION_DRAWS)
    keys["FMH_PACKED_UNROLL"] = ((None, "a depth"), None)
    for key, (values, _) in keys.items():
        mine = [c for c in cases if S.applies(c, key)]
        if key == "FMH_PACKED_UNROLL":
            assert sum(c.options().get(key) is None for c in mine) >= 2 and sum(c.options().get(key) is not None for c in mine) >= 2
            for c in mine:
                depth = c.options().get(key)
                assert depth is None or int(depth) in S.UNROLLS[c.lanes_per_row()]
            continue
        need = 1 if key == "FMH_TILED_BATCH" else 2  # (four values on the seeds that force the tiled route)
        for value in values:
            assert sum(c.options().get(key) == value for c in mine) >= need, (key, value)
    for case in cases:
        for key in S.BYTE_ROW_OPTIONS:
            assert key not in case.options() or not case.sweeps_packed, "set only where the header defines it"
        assert case.layout_at_sweep <= case.holds_both
    both = [c for c in cases if c.holds_both]
    assert sum(c.layout_at_sweep for c in both) >= 4 and sum(not c.layout_at_sweep for c in both) >= 4
    for origin in ("wrap-pack", "generate-pack", "regenerate"):
        assert any(c.layout_at_sweep for c in both if c.origin == origin), origin
    for pd_set in S.PD_SETS:
        assert sum(c.pd_set == pd_set for c in cases) >= 4, pd_set
    for own in (False, True):
        assert sum(c.own_stream == own for c in cases) >= 20
    for formulas in S.FUSED_FORMULAS:
        assert sum(c.fused == formulas for c in cases if c.pair is not None) >= 4, formulas
    assert all(S.SUMMARY not in c.fused and c.summaries_formula != S.SUMMARY for c in cases if c.max_allele > 1)
    # two forcing options at once, on a matrix that no fmh_matrix_create made
    crossed = [c for c in cases if c.origin != "create" and sum(S.applies(c, k) and c.options().get(k) not in (None, "-1") for k in S.OPTION_DRAWS) >= 3]
    assert len(crossed) >= 40, len(crossed)


def test_routes_windows_and_probes(cases):
    for name in ROUTES:
        assert sum(name in S.routes(c) for c in cases) >= 3, name
    assert sum("packed4_3p" in S.routes(c) or "packed16_3p" in S.routes(c) for c in cases if c.kind == "multi7") >= 6
    paired = [c for c in cases if c.pair is not None]
    windowed = [c for c in paired if c.sweeps_packed and c.plain and c.options()["FMH_COLUMN_WINDOW"] == "2" and not S.flat_wanted(c, 2)]
    assert sum(c.geometry in ("hull", "confined", "contiguous") for c in windowed) >= 3, "a window shorter than the row"
    # the probes: each assertion of the GPU test holds for six seeds or more
    assert sum(S.derives_a_group(c) for c in paired) >= 6
    assert sum(S.window_is_whole(c) and c.sweeps_packed for c in paired) >= 6
    assert sum(S.tiled_forced(c) for c in paired) >= 6
    assert sum(S.tiled_eligible(c) and c.options()["FMH_TILED"] == "0" for c in paired) >= 6
    assert sum(S.tiled_forced(c) and c.row_range == "inside" for c in paired) >= 2
    # the two tables only the sweeps read, on a matrix that was packed twice
    again = [c for c in cases if c.origin == "regenerate" and c.plain]
    assert sum(S.derives_a_group(c) for c in again) >= 1 and sum(S.tiled_forced(c) for c in again) >= 1


def test_the_junk_is_there(cases):
    """Set bits in plane 0 past the last column on the plane origins, junk under the uncalled entries of a general matrix on every origin
    that can carry it, and a wrapped matrix the byte kernels read as it is."""
    tails = 0
    for case in (c for c in cases if c.origin in ("planes", "planes-pitch")):
        planes, called_plane, pitch = S.plane_arrays(case)
        H, row_bytes = case.columns, (case.columns + 7) // 8
        spread = np.unpackbits(planes[0][:, :row_bytes], axis=1, bitorder="little")
        if case.max_allele <= 1 and H % 8:
            tails += 1
            assert spread[:, H:].any() and spread[0, H], "a set bit of plane 0 past the last column"
        else:
            assert not spread[:, H:].any()
        for plane in planes[1:] + ([] if called_plane is None else [called_plane]):
            assert not np.unpackbits(plane[:, :row_bytes], axis=1, bitorder="little")[:, H:].any(), "the other planes keep a zero tail"
    assert tails >= 4
    assert sum(S.derives_a_group(c) and c.origin in ("planes", "planes-pitch") and c.columns % 8 != 0 for c in cases) >= 1, "row_alt over a junk tail"
    general = [c for c in cases if c.max_allele > 1 and c.missing and c.pair is not None and c.origin not in F_GENERATED]
    for origin in ("planes", "planes-pitch", "wrap", "wrap-pack"):
        assert any(c.origin == origin for c in general), ("first_member_column over junk", origin)
    crowded = [c for c in general if c.kind.startswith(S.F.CROWDED) and c.sweeps_packed and c.origin in ("planes", "planes-pitch", "wrap-pack")]
    assert sum(c.row_count >= 60 for c in crowded) >= 1, "sites enough for an order of three products to show in the bits (one site in fifteen)"
    wrapped = [c for c in cases if c.origin == "wrap" or (c.origin == "wrap-pack" and c.layout_at_sweep)]
    assert sum(c.pitch > c.columns for c in wrapped) >= 6 and sum(c.missing and c.columns % 16 != 0 for c in wrapped) >= 3


F_GENERATED = S.F.GENERATED_ORIGINS


def test_what_runs(cases):
    for block in range(0, S.DEFAULT_CASES - 11, 12):
        twelve = cases[block:block + 12]
        assert sum("fused" in c.runs and "hudson" in c.runs for c in twelve) >= 11, block
        assert sum("wc" in c.runs for c in twelve) >= 11, block
    for case in cases:
        assert {"summaries", "pairwise", "pca_scan"} <= set(case.runs)
        assert ("hudson" in case.runs) == (case.columns >= 2) == ("wc" in case.runs)
        assert ("pca_gram" in case.runs) == (case.ploidy == 2 and case.columns <= S.GRAM_MAX_COLUMNS)
    assert sum("pca_gram" in c.runs for c in cases) >= 12
    assert sum(c.samples > S.PAIRWISE_MAX_SAMPLES for c in cases) >= 12 and sum(c.samples <= 2 for c in cases) >= 1
