"""The crossing fuzz of the sweeps, the pairwise differences and the PCA calls (tests/test_gpu_sweep_fuzz.py): what a seed draws, and the
matrix it builds.

draw(seed) fixes EVERY field of a case before any data is made - the origin of the matrix, the kind of cohort, its geometry, the row
range, the column groups, every library option and the formulas of the fused sweep - so that tests/test_sweep_fuzz_draws_cpu.py can
replay the draws without a device.  The cohorts, the plane images and the wrapped blocks are those of tests/cohort_fuzz.py (truth,
generated, plane_arrays, wrap_blocks, build), which this module calls.  This module imports no device.

Eight origins: the six of cohort_fuzz.ORIGINS and
  wrap          fmh_matrix_wrap of wrap_blocks(case) WITHOUT fmh_matrix_pack: the byte kernels, pd_planes_kernel and the byte route of
                the PCA scan read the caller's rows, whose padding columns, padding called-bits and bytes under uncalled entries are
                random over their full range.
  create-bytes  fmh_matrix_create with FMH_LAYOUT=bytes set while the matrix is made (and put back afterwards).
The two byte origins also meet a kind with max_allele = 9, which the planes cannot hold.

On the two plane origins of a biallelic kind the bits of plane 0 between the last column and the end of the row's last byte are random:
row_alt_kernel masks them (util_kernels.hpp: "fmh_matrix_create_packed takes the caller's planes as they are") and every sweep's masks
are zero there; no other table and no other plane is promised to.  (The called plane and the upper planes keep the zero tail the header
asks for: the packed kernels popcount the called plane and OR the upper planes whole.)

Two kinds of this fuzz's own, crowded3 and crowded7 (cohort_fuzz.crowded_cohort): the cohorts of tests/test_gpu_sfs.py carry an allele above
1 in a third of their rows and rarely three alleles that BOTH groups of a pair hold, so the order repair of the dense D_xy
(first_member_column) ran at a handful of sites per seed; in a crowded cohort it runs at nearly every site, with uncalled entries - and
under them, on the plane and wrap origins, junk - among a group's first members.  On the plane origins every second row holds ALL planes
set under its uncalled entries in place of random bits.

What is cycled and what is drawn.  With k = seed // 8: origin = seed % 8, kind = the origin's list at k % 12 (the biallelic complete
kind - the one the column window, the derived group, the tile-transposed image and the flat route need - every second time), the width
class = (k + k // 3) % 3, so every origin meets every kind and every width class within 96 seeds.  Everything else is drawn from
default_rng(SEED_BASE + seed), each option on its own; the weights lean towards the forcing values (FMH_COLUMN_WINDOW=2,
FMH_TILED_PLANES=2, FMH_TILED=1) because a probe or a route that needs three of them at once would else be met by a handful of seeds."""

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from tests import cohort_fuzz as F
from tests.test_gpu_sfs import KINDS as SFS_KINDS, missing_words, pack_rows

SEED_BASE = 52063  # the first base from 52000 on whose 96 default seeds meet every condition of tests/test_sweep_fuzz_draws_cpu.py
DEFAULT_CASES = 96
ORIGINS = F.ORIGINS + ("wrap", "create-bytes")
BYTE_ORIGINS = ORIGINS[6:]  # no packed image: u8 rows only
KINDS = dict(SFS_KINDS)
KINDS["multi9-missing"] = (9, True)
KINDS[F.CROWDED + "3"] = (3, True)  # cohort_fuzz.crowded_cohort: three shared alleles and more at nearly every site
KINDS[F.CROWDED + "7"] = (7, True)
KIND_CYCLE = ("complete", "missing", "complete", "crowded3", "complete", "multi7", "complete", "multi3-missing", "complete", "crowded7", "complete", "multi7")
BYTE_KIND_CYCLE = ("complete", "missing", "multi9-missing", "crowded3", "complete", "multi7", "complete", "multi3-missing", "multi9-missing", "crowded7", "complete", "multi7")
SAMPLES = [1, 2, 15, 17, 63, 65, 129, 257, 500, 1025, 2100, 2600]
ROWS = [1, 15, 17, 63, 65, 129, 257, 300]
WIDTHS = ("one-vector", "four-lane", "sixteen-lane")  # packed vectors of a row: 1, 2..32 (the flat route's width), more than 32
ROW_RANGES = ("whole", "inside")
GEOMETRIES = ("contiguous", "hull", "interleaved", "confined", "empty-group", "overlap")
GEOMETRY_WEIGHTS = (0.35, 0.17, 0.14, 0.12, 0.1, 0.12)
SPARSE, DENSE, SUMMARY = 0, 1, 2  # FMH_FORMULA_*
# (summary formula, Hudson formula or -1) of the fused sweep; SUMMARY is defined on biallelic matrices
FUSED_FORMULAS = ((SPARSE, SPARSE), (DENSE, SPARSE), (DENSE, -1), (SPARSE, -1), (DENSE, DENSE), (SUMMARY, SPARSE))
PD_SETS = ((), (("FMH_PD_INT8", "1"),), (("FMH_PD_TWO_PLANES", "1"),), (("FMH_PD_KCHUNK", "100000000"),), (("FMH_PD_SB", "32"),), (("FMH_PD_PHASED", "0"),))
PAIRWISE_MAX_SAMPLES = 400
GRAM_MAX_COLUMNS = 600
UNROLLS = {4: (1, 2, 3, 5), 16: (2, 3, 4)}  # sweep_plan.hpp: the batch depths built per lanes-per-row

# option -> (values, weights); None = left unset
OPTION_DRAWS = {
    "FMH_ROW_HI": (("0", "2", None), (1, 1, 1)),
    "FMH_COLUMN_WINDOW": (("0", "2"), (1, 3)),
    "FMH_TILED_PLANES": (("0", "2"), (3, 7)),
    "FMH_TILED": (("-1", "0", "1"), (2, 3, 5)),
    "FMH_TILED_BATCH": ((None, "10", "5", "2"), (1, 1, 1, 1)),
    "FMH_FLAT": (("-1", "0", "1"), (9, 4, 7)),
    "FMH_PACKED_LPR": ((None, "4", "16"), (1, 1, 1)),
    "FMH_PACKED_NO_PREFETCH": (("0", "1"), (1, 1)),
    "FMH_DEFER_TILES": ((None, "1", "2"), (1, 1, 1)),
    "FMH_WC_EXACT": (("0", "1"), (1, 1)),
    "FMH_GRID_BLOCKS": ((None, "1", "3"), (1, 1, 1)),
    "FMH_MASK_MODE": ((None, "2", "1"), (1, 1, 1)),
    "FMH_COUNTS_MFMA": (("0", "1", "2"), (1, 1, 1)),
}
BYTE_ROW_OPTIONS = ("FMH_MASK_MODE", "FMH_COUNTS_MFMA")  # defined for sweeps of u8 rows


@dataclass
class Case:
    seed: int
    origin: str
    kind: str
    max_allele: int
    missing: bool
    width: str
    ploidy: int
    samples: int
    rows: int
    columns: int
    release_bytes: bool
    extra: int                    # planes-pitch: host bytes per row beyond ceil(H / 8)
    pitch: int                    # wrap, wrap-pack: bytes per byte row
    bits_pitch: int               # wrap, wrap-pack: bytes per called bit-row
    row_range: str
    row_begin: int
    row_count: int
    geometry: str
    pair: Optional[np.ndarray]    # [2][columns] uint8, disjoint (None: fewer than two columns)
    wc: Optional[np.ndarray]      # [2..8][columns] uint8, disjoint (None: fewer than two columns)
    summary: np.ndarray           # [1..8][columns] uint8: wc, or overlapping masks, or the one column
    drawn: dict                   # every option as drawn, None = unset
    layout_at_sweep: bool         # FMH_LAYOUT=bytes from the first sweep on, on a matrix that holds both images
    pd_set: tuple
    own_stream: bool
    fused: tuple                  # (summary formula, Hudson formula or -1) of fmh_pair_region_sweep
    summaries_formula: int
    runs: tuple = field(default=())

    # ---- what the matrix holds and what a sweep reads ----
    @property
    def has_packed(self):
        return self.origin not in BYTE_ORIGINS

    @property
    def holds_both(self):
        return self.origin in ("wrap-pack", "regenerate") or (self.origin == "generate-pack" and not self.release_bytes)

    @property
    def sweeps_packed(self):  # plan_packed
        return self.has_packed and not self.layout_at_sweep

    @property
    def pvec(self):
        return (self.columns + 127) // 128

    @property
    def nvec(self):
        return (self.columns + 15) // 16

    @property
    def plain(self):  # biallelic, nothing missing: one plane and no called plane
        return self.max_allele <= 1 and not self.missing

    def options(self):
        """The options a test sets, before the matrix is made: the drawn ones the header defines for this matrix."""
        out = {}
        for key, value in self.drawn.items():
            if value is None or (key in BYTE_ROW_OPTIONS and self.sweeps_packed):
                continue
            out[key] = value
        return out

    def lanes_per_row(self):
        forced = self.options().get("FMH_PACKED_LPR")
        return int(forced) if forced else (4 if self.pvec <= 32 else 16)


def round_up(a, b):
    return (a + b - 1) // b * b


def width_class(columns):
    pvec = (columns + 127) // 128
    return WIDTHS[0] if pvec == 1 else WIDTHS[1] if pvec <= 32 else WIDTHS[2]


def kinds_of(origin):
    return BYTE_KIND_CYCLE if origin in BYTE_ORIGINS else KIND_CYCLE


def _choice(rng, values, weights):
    w = np.asarray(weights, dtype=np.float64)
    return values[int(rng.choice(len(values), p=w / w.sum()))]


def _span(H, lo, hi):
    return ((np.arange(H) >= lo) & (np.arange(H) < hi)).astype(np.uint8)


def _contiguous(rng, H, G, lo=0, hi=None):
    """G contiguous non-empty groups that tile [lo, hi)."""
    hi = H if hi is None else hi
    cuts = np.sort(rng.choice(np.arange(lo + 1, hi), size=G - 1, replace=False)) if G > 1 else np.zeros(0, dtype=np.int64)
    edges = [lo] + [int(c) for c in cuts] + [hi]
    return np.stack([_span(H, edges[g], edges[g + 1]) for g in range(G)])


def _interleaved(rng, H, G, support=None):
    """A random partition of `support` (default: every column) into G non-empty groups."""
    cols = np.arange(H) if support is None else np.nonzero(support)[0]
    owner = rng.integers(0, G, size=cols.size)
    owner[rng.permutation(cols.size)[:G]] = np.arange(G)
    out = np.zeros((G, H), dtype=np.uint8)
    out[owner, cols] = 1
    return out


def _groups(rng, geometry, H, G):
    """[G][H] disjoint masks of the geometry, or None where the row is too short for it."""
    if geometry == "contiguous":
        return _contiguous(rng, H, G)
    if geometry == "hull":  # ungrouped columns at both ends and one gap between two of the groups
        if H < G + 3 or G < 2:
            return None
        spare = H - G - 3
        lead, tail = 1 + int(rng.integers(0, spare // 3 + 1)), 1 + int(rng.integers(0, spare // 3 + 1))
        masks = _contiguous(rng, H, G, lead, H - tail)  # G + 1 columns or more: some group has two
        wide = [g for g in range(G) if masks[g].sum() >= 2]
        g = wide[int(rng.integers(0, len(wide)))]
        cols = np.nonzero(masks[g])[0]
        masks[g, cols[-1] if g < G - 1 else cols[0]] = 0  # the gap: between group g and a neighbour
        return masks
    if geometry == "interleaved":
        return _interleaved(rng, H, G)
    if geometry == "confined":  # members in the packed vectors 3..5 of the row only
        hi = min(H, 768)
        if hi - 384 < 2 * G:
            return None
        support = np.zeros(H, dtype=bool)
        support[384:hi] = rng.random(hi - 384) < 0.8
        support[384] = support[hi - 1] = True
        if support.sum() < G:
            return None
        return _interleaved(rng, H, G, support)
    if geometry == "empty-group":
        if G < 2:
            return None
        masks = _interleaved(rng, H, G - 1) if H >= G - 1 else None
        if masks is None:
            return None
        at = int(rng.integers(0, G))
        return np.insert(masks, at, 0, axis=0)
    raise ValueError(geometry)


def draw(seed):
    rng = np.random.default_rng(SEED_BASE + seed)
    k = seed // 8
    origin = ORIGINS[seed % 8]
    kind = kinds_of(origin)[k % 12]
    max_allele, missing = KINDS[kind]
    width = WIDTHS[(k + k // 3) % 3]
    shapes = [(p, s) for p in (1, 2, 3) for s in SAMPLES if width_class(p * s) == width]
    ploidy, samples = shapes[int(rng.integers(0, len(shapes)))]
    rows = int(rng.choice([r for r in ROWS if r >= 129] if kind.startswith(F.CROWDED) else ROWS))  # (the order repair shows in the bits of one site in fifteen)
    H = samples * ploidy
    row_bytes = (H + 7) // 8
    extras = [e for e in [1, 3, 16, 17] + ([0] if row_bytes % 16 else []) if row_bytes + e != round_up(row_bytes, 16)]
    extra = int(rng.choice(extras))
    pitch = round_up(H, 16) + int(rng.choice([0, 16, 48]))
    bits_pitch = round_up(round_up(H, 16) // 8, 4) + int(rng.choice([0, 4, 12]))
    release_bytes = bool(rng.integers(0, 2))

    # rows: whole, or a range with both ends off 16 (and so off the 64 rows of a tile)
    row_range = ROW_RANGES[int(rng.integers(0, 2))] if rows >= 3 else "whole"
    begins = [b for b in range(1, rows - 1) if b % 16]
    b = int(rng.choice(begins)) if begins else 0
    ends = [e for e in range(b + 1, rows + 1) if e % 16]
    e = int(rng.choice(ends)) if ends else rows
    row_begin, row_count = (b, e - b) if row_range == "inside" else (0, rows)

    # column groups: one geometry per seed; a row too short for it takes the interleaved partition
    geometry = _choice(rng, GEOMETRIES, GEOMETRY_WEIGHTS)
    G = min(int(rng.integers(2, 9)), H)
    pair = wc = None
    if H >= 2:
        partition = "interleaved" if geometry == "overlap" else geometry
        pair = _groups(rng, partition, H, 2)
        wc = _groups(rng, partition, H, G)
        if pair is None or wc is None:
            geometry = "interleaved"
            pair, wc = _interleaved(rng, H, 2), _interleaved(rng, H, G)
    overlapping = (rng.random((int(rng.integers(1, 9)), H)) < rng.choice([0.1, 0.5, 0.9])).astype(np.uint8)  # possibly empty groups
    overlapping[0, 0] = 1
    summary = overlapping if geometry == "overlap" or wc is None else wc

    drawn = {key: _choice(rng, values, weights) for key, (values, weights) in OPTION_DRAWS.items()}
    layout_draw = rng.random() < 0.35
    pd_set = PD_SETS[int(rng.integers(0, len(PD_SETS)))]
    own_stream = bool(rng.integers(0, 2))
    fused = [f for f in FUSED_FORMULAS if max_allele <= 1 or SUMMARY not in f]
    fused = fused[int(rng.integers(0, len(fused)))]
    summaries_formula = SUMMARY if max_allele <= 1 and rng.random() < 0.5 else DENSE
    unroll_draw = rng.random()

    case = Case(seed=seed, origin=origin, kind=kind, max_allele=max_allele, missing=missing, width=width, ploidy=ploidy, samples=samples, rows=rows,
                columns=H, release_bytes=release_bytes, extra=extra, pitch=pitch, bits_pitch=bits_pitch, row_range=row_range, row_begin=row_begin,
                row_count=row_count, geometry=geometry, pair=pair, wc=wc, summary=summary, drawn=drawn, layout_at_sweep=False, pd_set=pd_set,
                own_stream=own_stream, fused=fused, summaries_formula=summaries_formula)
    case.layout_at_sweep = bool(layout_draw and case.holds_both)
    # FMH_PACKED_UNROLL: unset, or one depth the lanes-per-row of this matrix is built with
    depths = UNROLLS[case.lanes_per_row()]
    drawn["FMH_PACKED_UNROLL"] = None if unroll_draw < 1 / 3 else str(depths[int((unroll_draw - 1 / 3) * 1.5 * len(depths)) % len(depths)])
    case.runs = ("summaries", "pairwise", "pca_scan") + (("hudson", "fused", "wc") if H >= 2 else ()) + (("pca_gram",) if ploidy == 2 and H <= GRAM_MAX_COLUMNS else ())
    return case


# ---- what the plan of a sweep must be (ferromic_amd/csrc/sweep_plan.hpp), from the draw alone ------------------------------------------------
WC, NOT_WC = "wc", "other"


def flat_wanted(case, n_groups, mode=NOT_WC):
    """plan_flat_wanted: the flat route pre-empts the window and the tiled route.  FMH_FLAT_BUILDS: one, two and four (padded) groups of
    summaries, two and four of W&C, one and two of the pair sweeps - every call of this fuzz with at most four groups."""
    assert mode in (WC, NOT_WC)
    return case.sweeps_packed and case.plain and case.pvec <= 32 and n_groups <= 4 and case.options().get("FMH_FLAT") == "1"


def window_is_whole(case):
    """fmh_sweep_window answers (0, vectors of the row, -1)."""
    return not case.sweeps_packed or case.options().get("FMH_COLUMN_WINDOW") == "0" or not case.plain


def window_vectors(case):
    return case.pvec if case.sweeps_packed else case.nvec


def derives_a_group(case):
    """A contiguous two-group partition of a plain packed matrix of two vectors or more under FMH_COLUMN_WINDOW=2: one group's vectors are
    skipped (a cut at column c leaves group 0 the vectors 0 .. (c - 1) // 128 and group 1 the vectors c // 128 .. - one of the two ranges is
    shorter than the row)."""
    return (case.sweeps_packed and case.plain and case.pvec >= 2 and case.geometry == "contiguous" and case.pair is not None
            and case.options().get("FMH_COLUMN_WINDOW") == "2" and not flat_wanted(case, 2))


def tiled_eligible(case):
    """The matrix holds the tile-transposed image and a sweep of one or two groups may read it."""
    return case.sweeps_packed and case.plain and case.options().get("FMH_TILED_PLANES") == "2" and not flat_wanted(case, 2)


def tiled_forced(case):
    return tiled_eligible(case) and case.options().get("FMH_TILED") == "1"


def route(case, n_groups, mode=NOT_WC, fused_region=False):
    """The SweepRoute of a sweep of n_groups groups, where the draw alone decides it (None: it depends on the window, i.e. on FMH_TILED=-1)."""
    opts = case.options()
    padded = 1 if n_groups <= 1 else 2 if n_groups <= 2 else 4 if n_groups <= 4 else 8
    if case.sweeps_packed:
        if mode != WC and n_groups <= 2 and tiled_eligible(case):
            if opts.get("FMH_TILED") == "1":
                return "tiled"
            if opts.get("FMH_TILED") == "-1":
                return None
        if flat_wanted(case, n_groups, mode):
            return "flat"
        lanes = case.lanes_per_row()
        return f"packed{lanes}_3p" if case.max_allele >= 4 else f"packed{lanes}"
    if not (fused_region and padded == 2) and opts.get("FMH_COUNTS_MFMA", "0") != "0" and case.plain and padded <= 4:
        return "mfma"
    if opts.get("FMH_MASK_MODE") == "1" and padded <= 2 and mode != WC:
        return "global"
    return "bits" if opts.get("FMH_MASK_MODE") == "2" else "bytes"


def routes(case):
    """Every route the draw fixes for the sweeps of this case."""
    out = {route(case, case.summary.shape[0])}
    if case.pair is not None:
        out |= {route(case, 2), route(case, 1), route(case, 2, fused_region=True), route(case, case.wc.shape[0], WC)}
    return out - {None}


def applies(case, key):
    """Whether the option `key`, at a forcing value, changes what the library does with this case's matrix (the preconditions of
    sweep_plan.hpp and of the builders of the tables in abi.hip)."""
    lanes = case.lanes_per_row()
    if key == "FMH_ROW_HI":
        return case.has_packed and not case.plain
    if key in ("FMH_COLUMN_WINDOW", "FMH_TILED_PLANES"):
        return case.has_packed and case.plain
    if key == "FMH_TILED":
        return tiled_eligible(case)
    if key == "FMH_TILED_BATCH":
        return tiled_forced(case)
    if key == "FMH_FLAT":
        return case.sweeps_packed and case.plain and case.pvec <= 32
    if key in ("FMH_PACKED_LPR", "FMH_PACKED_UNROLL", "FMH_PACKED_NO_PREFETCH"):
        return case.sweeps_packed
    if key == "FMH_DEFER_TILES":  # defer_rule: biallelic kernels of sixteen lanes per row (u8 rows always are)
        return case.max_allele <= 1 and (not case.sweeps_packed or lanes == 16)
    if key == "FMH_WC_EXACT":
        return case.sweeps_packed and case.plain and case.wc is not None and 5 <= case.wc.shape[0] <= 7
    if key == "FMH_GRID_BLOCKS":
        return True
    if key == "FMH_MASK_MODE":
        return not case.sweeps_packed
    if key == "FMH_COUNTS_MFMA":
        return not case.sweeps_packed and case.plain
    raise KeyError(key)


# ---- host images ---------------------------------------------------------------------------------------------------------------------------
def truth(case):
    return F.truth(case)


def plane_arrays(case):
    """cohort_fuzz.plane_arrays, and on a biallelic kind random bits in plane 0 from the last column to the end of the row's last byte."""
    planes, called_plane, pitch = F.plane_arrays(case)
    H = case.columns
    if called_plane is not None:
        # every second row: ALL planes set under the uncalled entries (a host that fills missing calls with 0xFF) in place of random bits.
        # The highest allele is the rarest, so its first called carrier sits far into a group: an uncalled entry before it that passes for
        # one moves that allele forward in the first-occurrence order of the dense D_xy (first_member_column).
        _, called = truth(case)
        fill = pack_rows((~called) & (np.arange(case.rows) % 2 == 1)[:, None], pitch)
        planes = [plane | fill for plane in planes]
    if case.max_allele <= 1 and H % 8:
        rng = np.random.default_rng(SEED_BASE + 70000 + case.seed)
        junk = rng.integers(0, 256, size=case.rows, dtype=np.uint8) & np.uint8((0xFF << (H % 8)) & 0xFF)
        junk[0] |= np.uint8(1 << (H % 8))
        planes[0] = planes[0].copy()
        planes[0][:, (H + 7) // 8 - 1] |= junk
    return planes, called_plane, pitch


def build(dev, case):
    """(dm, x, called, keepalive) as cohort_fuzz.build.  The options of the case are set by the caller, before."""
    from ferromic_amd import _abi

    rows, samples, ploidy, max_allele = case.rows, case.samples, case.ploidy, case.max_allele
    if case.origin in ("planes", "planes-pitch"):
        x, called = truth(case)
        planes, called_plane, _ = plane_arrays(case)
        return dev.DeviceMatrix.from_host_planes(planes, called_plane, rows, samples, ploidy, max_allele), x, called, []
    if case.origin == "wrap":
        x, called = truth(case)
        dm, keepalive = F.wrap(dev, case, pack=False)
        return dm, x, called, keepalive
    if case.origin == "create-bytes":
        x, called = truth(case)
        data = x if called is None else np.where(called, x, 0).astype(np.uint8)
        with _abi.options(FMH_LAYOUT="bytes"):
            dm = dev.DeviceMatrix.from_host(data, None if called is None else missing_words(called), rows, samples, ploidy, max_allele)
        return dm, x, called, []
    return F.build(dev, case)
