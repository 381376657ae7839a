"""The crossing fuzz of the nine cohort statistics (tests/test_gpu_cohort_fuzz.py): what a seed draws, and the matrix it builds.

draw(seed) fixes EVERY field of a case before any data is made - the route the matrix takes onto the device (ORIGINS), the kind of cohort,
its geometry, the library options and the arguments of every statistic's call - so that tests/test_cohort_fuzz_draws_cpu.py can replay the
draws without a device and show that the default seeds cover what they claim.  truth(case) makes the host cohort of the four origins whose
data the host makes, generated(case) the cohort of the two whose data the device's generator makes (the same counter-based hash in numpy
uint64), and build(dev, case) puts either on the device through the case's route.  This module imports no device.

The six origins:
  create         fmh_matrix_create.
  planes         fmh_matrix_create_packed at the device's own pitch, random bits under the uncalled entries of every allele plane.
  planes-pitch   fmh_matrix_create_packed at a foreign h_pitch (the memset + pitched-copy branch): rows of ceil(H / 8) + extra bytes, the
                 host bytes from ceil(H / 8) on are 0xFF and must not reach the device; the bits past the last column inside byte
                 ceil(H / 8) - 1 are zero, the caller's contract in include/ferromic_hip.h.
  wrap-pack      fmh_matrix_wrap of caller-owned byte rows and called bit-rows, then fmh_matrix_pack.  Padding bytes (columns H .. pitch),
                 padding called-bits (bits H .. 8 bits_pitch) and the bytes under uncalled entries are random over their FULL range, bits
                 above max_allele included: the header asks only that CALLED entries stay within max_allele, and the library does take all
                 of it (nothing had to be narrowed).
  generate-pack  fmh_matrix_alloc, fmh_matrix_generate, fmh_matrix_pack (with or without release_bytes).
  regenerate     the same, then fmh_matrix_generate of the case's cohort on the packed matrix, which re-packs it in place.  The first
                 generation has nothing missing, so its row_gap table marks every row clean: a table that is not rebuilt hides every
                 uncalled entry of the second.

FMH_ROW_HI goes by (seed // 6) % 3: with origin = seed % 6 every origin meets every setting within the default 48 seeds."""

import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from tests.helpers import thresholds
from tests.test_gpu_assoc import values_for
from tests.test_gpu_sfs import KINDS, cohort, missing_words, pack_rows

SEED_BASE = 31014  # the first base from 31000 on whose 48 default seeds meet every condition of tests/test_cohort_fuzz_draws_cpu.py
DEFAULT_CASES = 48
ORIGINS = ("create", "planes", "planes-pitch", "wrap-pack", "generate-pack", "regenerate")
HOST_ORIGINS = ORIGINS[:4]
GENERATED_ORIGINS = ORIGINS[4:]  # (tests/sweep_fuzz.py adds origins of its own whose data the host makes)
SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 500, 1025, 1300]
ROWS = [1, 15, 17, 63, 65, 129, 257, 300, 600]
ROW_HI = ("0", "2", None)
GRID_BLOCKS = (None, "1", "3")
ITEM_ROWS = (None, "16", "48")
ITEM_ROWS_KEYS = ("FMH_ASSOC_ITEM_ROWS", "FMH_QC_ITEM_ROWS", "FMH_FSTAT_ITEM_ROWS")
SAMPLE_LISTS = ("none", "prefix", "every-second", "random-30%", "last-nine")
ROW_RANGES = ("whole", "inside")
KEEP_MASKS = ("none", "random-70%", "all-but-one")
LD_MASKS = ("none", "half", "confined")
VALUE_COLUMNS = (1, 5, 17)
LD_BANDS = (1, 33, 70)
LD_THRESHOLD = 0.3
KINSHIP_MAX_SAMPLES = 400
MISSING_THRESHOLD24 = 67109  # 0.4 % of 2^24
COLUMN_STATISTICS = ("ld", "sfs", "sfs_joint", "haplotype_windows", "ehh", "fstat")
DIPLOID_STATISTICS = ("kinship", "qc", "assoc", "homalt")
STATISTICS = COLUMN_STATISTICS + DIPLOID_STATISTICS


@dataclass
class Case:
    seed: int
    origin: str
    kind: str
    max_allele: int
    missing: bool
    ploidy: int
    samples: int
    rows: int
    columns: int
    release_bytes: bool
    row_hi: Optional[str]
    grid_blocks: Optional[str]
    item_rows: Optional[str]
    own_stream: bool
    extra: int                  # planes-pitch: host bytes per row beyond ceil(H / 8)
    pitch: int                  # wrap-pack: bytes per byte row
    bits_pitch: int             # wrap-pack: bytes per called bit-row
    sample_list: str
    sel: Optional[np.ndarray]   # the selected sample numbers, ascending (None: all)
    as_prefix: bool             # sel is passed as n_samples, not as a list
    kin_sel: Optional[np.ndarray]
    kin_prefix: bool
    row_range: str
    row_begin: int
    row_count: int
    keep_mask: str
    keep: Optional[np.ndarray]  # [row_count] uint8
    half: np.ndarray            # [columns] bool, a random 50 %
    confined: Optional[np.ndarray]  # members in the 16-byte vectors 3..5 of a row only, when the row has them
    ld_mask: str
    pair: Optional[np.ndarray]  # [2][columns] bool, a partition (None: fewer than 2 columns)
    groups: Optional[np.ndarray]  # [G][columns] bool, a partition into 3..9
    windows: list
    focal: list
    value_columns: int
    band: int
    prune_chunk: int
    runs: tuple = field(default=())

    def options(self):
        out = {"FMH_ROW_HI": self.row_hi, "FMH_GRID_BLOCKS": self.grid_blocks}
        out.update({key: self.item_rows for key in ITEM_ROWS_KEYS})
        return {k: v for k, v in out.items() if v is not None}


def round_up(a, b):
    return (a + b - 1) // b * b


def _partition(rng, cols, G):
    order = rng.permutation(cols)
    owner = rng.integers(0, G, size=cols)
    owner[order[:G]] = np.arange(G)  # no group is empty
    return np.stack([owner == g for g in range(G)])


def draw(seed):
    rng = np.random.default_rng(SEED_BASE + seed)
    origin = ORIGINS[seed % 6]
    kind = list(KINDS)[(seed // 6) % 4]
    max_allele, missing = KINDS[kind]
    ploidy = 1 if seed % 8 == 3 else 3 if seed % 8 == 7 else 2
    samples = int(rng.choice(SAMPLES))
    rows = int(rng.choice(ROWS))
    H = samples * ploidy
    row_bytes = (H + 7) // 8
    # never the device's own pitch: there the header wants the padding bytes zero, and the 0xFF would be counted (125 + 3 = 128 at 1 000 columns)
    extras = [e for e in [1, 3, 16, 17] + ([0] if row_bytes % 16 else []) if row_bytes + e != round_up(row_bytes, 16)]
    extra = int(rng.choice(extras))
    pitch = round_up(H, 16) + int(rng.choice([0, 16, 48]))
    bits_pitch = round_up(round_up(H, 16) // 8, 4) + int(rng.choice([0, 4, 12]))
    grid_blocks = GRID_BLOCKS[int(rng.integers(0, 3))]
    item_rows = ITEM_ROWS[int(rng.integers(0, 3))]

    # the samples of the diploid calls
    sample_list = SAMPLE_LISTS[int(rng.integers(0, 5))] if samples >= 2 else "none"
    prefix_n = int(rng.integers(1, max(samples, 2)))
    thirty = np.sort(rng.choice(samples, size=max(1, int(round(0.3 * samples))), replace=False))
    sel = {"none": None, "prefix": np.arange(prefix_n), "every-second": np.arange(0, samples, 2), "random-30%": thirty,
           "last-nine": np.arange(max(0, samples - 9), samples)}[sample_list]
    as_prefix = sample_list == "prefix"
    kin_sel, kin_prefix = sel, as_prefix
    if (samples if sel is None else sel.size) > KINSHIP_MAX_SAMPLES:  # the oracle's n^2 tables: kinship takes a prefix or a shorter list
        n = int(rng.integers(257, KINSHIP_MAX_SAMPLES + 1))
        kin_sel, kin_prefix = (np.arange(n), True) if sel is None or as_prefix else (sel[:n], False)

    # rows: whole, or a range with both ends off 16
    row_range = ROW_RANGES[int(rng.integers(0, 2))] if rows >= 3 else "whole"
    begins = [b for b in range(1, rows - 1) if b % 16]
    b = int(rng.choice(begins)) if begins else 0
    ends = [e for e in range(b + 1, rows + 1) if e % 16]
    e = int(rng.choice(ends)) if ends else rows
    row_begin, row_count = (b, e - b) if row_range == "inside" else (0, rows)
    keep_mask = KEEP_MASKS[int(rng.integers(0, 3))]
    seventy = (rng.random(row_count) < 0.7).astype(np.uint8)
    but_one = np.ones(row_count, dtype=np.uint8)
    but_one[int(rng.integers(0, row_count))] = 0
    keep = {"none": None, "random-70%": seventy, "all-but-one": but_one}[keep_mask]

    # column groups
    half = rng.random(H) < 0.5
    half[int(rng.integers(0, H))] = True
    confined = None
    if H > 384:
        hi = min(H, 768)
        confined = np.zeros(H, dtype=bool)
        confined[384:hi] = rng.random(hi - 384) < 0.8
        confined[384] = confined[hi - 1] = True
    ld_mask = LD_MASKS[int(rng.integers(0, 3))]
    if ld_mask == "confined" and confined is None:
        ld_mask = "half"
    G = min(int(rng.integers(3, 10)), H)
    pair = _partition(rng, H, 2) if H >= 2 else None
    groups = _partition(rng, H, G) if G >= 2 else None

    # three row ranges for the windowed statistics: an empty one, one to the last row, one anywhere - in a drawn order
    a = int(rng.integers(0, rows + 1))
    c = int(rng.integers(0, rows))
    lo, hi = sorted(int(v) for v in rng.integers(0, rows + 1, size=2))
    windows = [(a, a), (c, rows), (lo, hi)]
    windows = [windows[i] for i in rng.permutation(3)]
    focal = sorted({row_begin, row_begin + row_count - 1, int(rng.integers(row_begin, row_begin + row_count))})
    value_columns = int(rng.choice(VALUE_COLUMNS))
    band = int(rng.choice(LD_BANDS))
    prune_chunk = int(rng.choice([0, 77]))

    runs = ["ld", "sfs", "haplotype_windows", "ehh"] + (["sfs_joint"] if pair is not None else []) + (["fstat"] if groups is not None else [])
    if ploidy == 2:
        runs += list(DIPLOID_STATISTICS)
    return Case(seed=seed, origin=origin, kind=kind, max_allele=max_allele, missing=missing, ploidy=ploidy, samples=samples, rows=rows, columns=H,
                release_bytes=bool((seed // 6) % 2), row_hi=ROW_HI[(seed // 6) % 3], grid_blocks=grid_blocks, item_rows=item_rows,
                own_stream=bool((seed // 2) % 2), extra=extra, pitch=pitch, bits_pitch=bits_pitch, sample_list=sample_list, sel=sel, as_prefix=as_prefix,
                kin_sel=kin_sel, kin_prefix=kin_prefix, row_range=row_range, row_begin=row_begin, row_count=row_count, keep_mask=keep_mask, keep=keep,
                half=half, confined=confined, ld_mask=ld_mask, pair=pair, groups=groups, windows=windows, focal=focal, value_columns=value_columns,
                band=band, prune_chunk=prune_chunk, runs=tuple(s for s in STATISTICS if s in runs))


def ld_column_mask(case):
    return {"none": None, "half": case.half, "confined": case.confined}[case.ld_mask]


def sample_arguments(sel, as_prefix):
    """(samples, n_samples) as the device calls take them."""
    if sel is None:
        return None, None
    return (None, int(sel.size)) if as_prefix else (sel, None)


def values(case):
    n = case.samples if case.sel is None else int(case.sel.size)
    return values_for(n, case.value_columns, case.seed)


# ---- host cohorts ------------------------------------------------------------------------------------------------------------------------
CROWDED = "crowded"  # prefix of the kinds of tests/sweep_fuzz.py whose cohort is crowded_cohort


@functools.lru_cache(maxsize=None)
def crowded_cohort(rows, cols, max_allele, seed):
    """(x, called) with every allele 0 .. max_allele equally common in every row and three entries in ten uncalled (every fourth row is
    complete): both groups of a pair carry three alleles and more at nearly every site, and the first members of a group are often
    uncalled - the sites at which the dense D_xy is added in first-occurrence order (sweep_kernels.hpp, first_member_column)."""
    rng = np.random.default_rng(2000003 * rows + 7919 * cols + 31 * max_allele + seed)
    x = rng.integers(0, max_allele + 1, size=(rows, cols), dtype=np.uint8)
    called = rng.random((rows, cols)) >= 0.3
    called[::4] = True
    x[0, 0] = max_allele
    x.setflags(write=False)
    called.setflags(write=False)
    return x, called


def truth(case):
    """(x [rows][columns] uint8, called [rows][columns] bool or None) of an origin whose data the host makes; read-only and shared."""
    assert case.origin not in GENERATED_ORIGINS
    if case.kind.startswith(CROWDED):
        return crowded_cohort(case.rows, case.columns, case.max_allele, case.seed)
    return cohort(case.rows, case.columns, case.max_allele, case.missing, seed=case.seed)


def _hash24(seed, site, column):
    """The splitmix64 finaliser of the library's counter-based generator, on numpy uint64 (wrapping) arrays."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = u(seed) + u(0x9E3779B97F4A7C15) * (site * u(0x100000001B3) + column + u(1))
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(40)).astype(np.uint32)


def host_generate(rows, columns, seed, thresholds24, pop_of_column, missing_threshold24):
    """What fmh_matrix_generate writes (include/ferromic_hip.h): (x [rows][columns] uint8, called [rows][columns] bool)."""
    site = np.arange(rows, dtype=np.uint64)[:, None]
    column = np.arange(columns, dtype=np.uint64)[None, :]
    thr = np.asarray(thresholds24, dtype=np.uint32)[np.asarray(pop_of_column, dtype=np.int64)].T  # [rows][columns]
    bit = _hash24(seed, site, column) < thr
    miss = _hash24(seed ^ 0xA5A5A5A5DEADBEEF, site, column) < np.uint32(missing_threshold24)
    return (bit & ~miss).astype(np.uint8), ~miss


def generator_arguments(case, first=False):
    """(seed, thresholds [2][rows], pop_of_column [columns], missing threshold) of the case's cohort, or (first=True) of the generation a
    `regenerate` case packs before it: another seed, nothing missing."""
    seed = 7919 * case.seed + (104729 if first else 13)
    poc = (np.arange(case.columns) >= case.columns // 2).astype(np.uint8)
    return seed, thresholds(case.rows, seed), poc, (MISSING_THRESHOLD24 if case.missing and not first else 0)


def generated(case, first=False):
    """(x, called or None) of a generate-pack / regenerate case from the host twin of the generator."""
    assert case.origin in GENERATED_ORIGINS
    x, called = host_generate(case.rows, case.columns, *generator_arguments(case, first))
    return x, (called if case.missing else None)


# ---- the host images of the plane and wrap origins -----------------------------------------------------------------------------------------
def plane_arrays(case):
    """(allele planes, called plane or None, h_pitch) of a planes / planes-pitch case."""
    x, called = truth(case)
    rng = np.random.default_rng(SEED_BASE + 50000 + case.seed)
    n_planes = 1 if case.max_allele <= 1 else 2 if case.max_allele <= 3 else 3
    stored = x
    if called is not None:  # random bits under the uncalled entries of every allele plane
        stored = np.where(called, x, rng.integers(0, 1 << n_planes, size=x.shape, dtype=np.uint8)).astype(np.uint8)
    row_bytes = (case.columns + 7) // 8
    pitch = round_up(row_bytes, 16) if case.origin == "planes" else row_bytes + case.extra

    def lay(bits):
        plane = pack_rows(bits, pitch)
        if case.origin == "planes-pitch":
            plane[:, row_bytes:] = 0xFF  # beyond the row: not the library's to read
        return plane

    return [lay((stored >> k) & 1) for k in range(n_planes)], None if called is None else lay(called), pitch


def wrap_blocks(case):
    """(byte rows [rows][pitch] uint8, called bit-rows [rows][bits_pitch] uint8 or None) of a wrap-pack case: junk over the full range in
    the padding and under the uncalled entries; the first padding byte and the first padding bit of row 0 are set outright."""
    x, called = truth(case)
    H = case.columns
    rng = np.random.default_rng(SEED_BASE + 60000 + case.seed)
    block = rng.integers(0, 256, size=(case.rows, case.pitch), dtype=np.uint8)
    block[:, :H] = x if called is None else np.where(called, x, block[:, :H])
    if case.pitch > H:
        block[0, H] = 0xFF
    if called is None:
        return block, None
    bits = rng.integers(0, 2, size=(case.rows, case.bits_pitch * 8), dtype=np.uint8)
    bits[:, :H] = called
    if case.bits_pitch * 8 > H:
        bits[0, H] = 1
    return block, np.packbits(bits, axis=1, bitorder="little")


def unmasked_planes(case):
    """(plane 0 [rows][pitch / 8], called plane [rows][bits_pitch] or None) of a wrap-pack case packed with NO column mask: what a
    padding-blind pack would have written."""
    block, bits = wrap_blocks(case)
    return np.packbits(block & 1, axis=1, bitorder="little"), bits


# ---- onto the device -----------------------------------------------------------------------------------------------------------------------
def _downloaded(dm, case):
    data, words = dm.download()
    x = data.reshape(case.rows, case.columns)
    if words is None:
        return x, None
    miss = np.unpackbits(words.view(np.uint8), bitorder="little")[: x.size].reshape(x.shape).astype(bool)
    return x, ~miss


def wrap(dev, case, pack):
    """(dm, keepalive): fmh_matrix_wrap of wrap_blocks(case) uploaded into device blocks of the test's own, then (pack) fmh_matrix_pack."""
    block, bits = wrap_blocks(case)
    keepalive = [dev.DeviceBuffer.from_numpy(0, block)] + ([] if bits is None else [dev.DeviceBuffer.from_numpy(0, bits)])
    try:
        dm = dev.DeviceMatrix.wrap(keepalive[0].ptr, case.pitch, None if bits is None else keepalive[1].ptr, 0 if bits is None else case.bits_pitch,
                                   case.rows, case.samples, case.ploidy, case.max_allele)
        if pack:
            dm.pack()
    except Exception:
        for b in keepalive:
            b.free()
        raise
    return dm, keepalive


def build(dev, case):
    """(dm, x, called, keepalive): the case's matrix made through its origin, and the cohort it holds.  For the generated origins the
    cohort is the matrix's own download - before the pack of generate-pack, when the matrix still answers with its byte rows.  keepalive
    holds the device blocks a wrapped matrix points into; free them after the matrix."""
    rows, samples, ploidy, max_allele = case.rows, case.samples, case.ploidy, case.max_allele
    keepalive = []
    if case.origin == "create":
        x, called = truth(case)
        data = x if called is None else np.where(called, x, 0).astype(np.uint8)
        dm = dev.DeviceMatrix.from_host(data, None if called is None else missing_words(called), rows, samples, ploidy, max_allele)
    elif case.origin in ("planes", "planes-pitch"):
        x, called = truth(case)
        planes, called_plane, _ = plane_arrays(case)
        dm = dev.DeviceMatrix.from_host_planes(planes, called_plane, rows, samples, ploidy, max_allele)
    elif case.origin == "wrap-pack":
        x, called = truth(case)
        dm, keepalive = wrap(dev, case, pack=True)
    else:
        dm = dev.DeviceMatrix.alloc(rows, samples, ploidy, case.missing, max_allele)
        try:
            if case.origin == "regenerate":
                seed, thr, poc, _ = generator_arguments(case, first=True)
                dm.generate(seed, 0, thr, poc, 0)
                dm.pack()
            seed, thr, poc, missing_thr = generator_arguments(case)
            dm.generate(seed, 0, thr, poc, missing_thr)  # regenerate: on the packed matrix, which the library re-packs
            x, called = _downloaded(dm, case)
            if case.origin == "generate-pack":
                dm.pack(case.release_bytes)
        except Exception:
            dm.close()
            raise
    return dm, x, called, keepalive


def stream_handle(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)
