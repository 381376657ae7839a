"""Genotype QC on the device (fmh_genotype_counts, fmh_hwe_exact) against tests/qc_ref.py, the numpy oracle written from the definition.
Every table is compared with array_equal on integers; every f64 bitwise with the oracle, NaN positions equal.  Cohorts and uploads are
test_gpu_sfs.py's (random bits under the uncalled entries of every allele plane), with ploidy 2.

Shapes are the smallest at which each part of the kernels can go wrong:
  * samples around a 32-bit word (15 .. 17), a 128-column vector (63 .. 65), every change of the word-lane count LW (8 lanes up to 128
    samples, then 16, 32, 64, 128, 256 lanes: 128/129, 256/257, 512/513, 1 024/1 025 - one wave's worth of words -, 2 048/2 049) and the cut
    into column chunks (4 096/4 097; 4 100: more words than one 256-thread step covers), in matrices of n and of n + 3 samples;
  * rows around the 8 rows of a carry-save block, the rows of a pass (8 x 256 / LW: 256 at 34 samples) and the 4 096 rows of an item;
  * rows around what a lane's bit-sliced counters hold before they are emptied: 31 blocks of 8 = 248 rows of a LANE, which is 248 x 32 =
    7 936 rows of an item at 34 samples (8 word lanes x 32 row lanes; FMH_QC_ITEM_ROWS raised so that an item is that long) and 248 rows at
    2 100 samples (256 word lanes, one row lane).  Sample 0 is het, sample 1 hom-alt and sample 2 uncalled at every row there: a counter that
    wraps or is emptied late shows as count != rows.
Preconditions are asserted on the oracle alone, before the device is called, so that a transposed, mask-blind or keep-blind kernel cannot
pass."""

import ctypes as C

import numpy as np
import pytest

from tests import kinship_ref, qc_ref
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024, 1025]
WIDE_SAMPLES = [2048, 2049, 4096, 4097, 4100]   # about 70 rows there
ROWS = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
CLASSES = ("hom_ref", "het", "hom_alt")
SPECIAL_WEIGHTS = [0, 1, 1 << 31, (1 << 32) - 1]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def row_weights(rows, seed=0):
    """u32 weights that contain 0, 1, 2^31 and 2^32 - 1 (as many of them as there are rows)."""
    w = np.random.default_rng(rows + seed).integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)
    w[: min(rows, 4)] = SPECIAL_WEIGHTS[: min(rows, 4)]
    return w


def preconditions(kind, x, called, samples=None, weights=None):
    """What makes a wrong kernel visible, from the oracle alone (cohorts of >= 64 rows and >= 15 samples)."""
    max_allele, missing = KINDS[kind]
    site = qc_ref.site_tracks(x, called, samples)
    table = qc_ref.sample_tables(x, called, samples)
    n = table[0].size
    for a in range(3):
        assert np.unique(site[a]).size > 1, "a track differs between rows"
        assert np.unique(table[a]).size > 1, "a table differs between samples"
        for b in range(a):
            assert (site[a] != site[b]).any() and (table[a] != table[b]).any(), "the classes differ from each other"
    N = site[0].astype(np.int64) + site[1] + site[2]
    c, _ = qc_ref.classes(x, called, samples)
    if missing:
        assert (N < n).any(), "a missing call lowers some N"
    if max_allele > 1:
        high = x > 1
        if called is not None:
            high = high & called
        pairs = high.reshape(x.shape[0], -1, 2).any(axis=2)
        assert (pairs if samples is None else pairs[:, np.asarray(samples)]).any(), "an upper allele plane un-calls some genotype"
    if weights is not None and (missing or max_allele > 1):
        assert (qc_ref.weighted_called(x, called, weights, samples) < int(weights.astype(np.uint64).sum())).any(), "some weighted sum is below the total"


def check(dev, dm, x, called, what, samples=None, n_samples=None, row_begin=0, row_count=None, keep=None, weights=None, stream=None):
    """One device call (tracks, tables and - with `weights` - the weighted sum at once) against the oracle; returns the device's result."""
    rows = x.shape[0] - row_begin if row_count is None else row_count
    sel = samples if samples is not None else (None if n_samples is None else np.arange(n_samples))
    xs = x[row_begin : row_begin + rows]
    cs = None if called is None else called[row_begin : row_begin + rows]
    got = dev.genotype_counts(dm, samples=samples, n_samples=n_samples, row_begin=row_begin, row_count=rows, keep=keep, weights=weights, stream=stream,
                              fill=0xA5)
    for name, ref in zip(CLASSES, qc_ref.site_tracks(xs, cs, sel)):
        g = got.site[name]
        assert g.dtype == np.uint32 and g.shape == ref.shape, (what, "site", name)
        assert np.array_equal(g, ref), (what, "site", name, np.flatnonzero(g != ref)[:4].tolist())
    for name, ref in zip(CLASSES, qc_ref.sample_tables(xs, cs, sel, keep)):
        g = got.sample[name]
        assert g.dtype == np.uint64 and g.shape == ref.shape, (what, "sample", name)
        assert np.array_equal(g, ref), (what, "sample", name, np.flatnonzero(g != ref)[:4].tolist())
    if weights is not None:
        ref = qc_ref.weighted_called(xs, cs, weights, sel, keep)
        assert np.array_equal(got.sample["weighted_called"], ref), (what, "weighted", np.flatnonzero(got.sample["weighted_called"] != ref)[:4].tolist())
    assert got.kept_rows == (rows if keep is None else int(np.count_nonzero(keep))), what
    return got


# ---- samples: word, vector, lane-count and chunk edges; every kind; both upload forms --------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["from_host", "from_host_planes"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_sample_count(dev, kind, planes):
    max_allele, missing = KINDS[kind]
    for n in SAMPLES + WIDE_SAMPLES:
        rows = 257 if n <= 1025 else 70
        weights = row_weights(rows)
        for extra in (0, 3):
            x, called = cohort(rows, 2 * (n + extra), max_allele, missing, seed=5)
            if n >= 15:
                preconditions(kind, x, called, None if extra == 0 else np.arange(n), weights)
            dm = upload(dev, x, called, max_allele, planes, ploidy=2)
            try:
                check(dev, dm, x, called, (kind, planes, n, extra), n_samples=n, weights=weights)
            finally:
                dm.close()


# ---- rows: block, pass, item and counter-capacity edges -------------------------------------------------------------------------------------
def marked_cohort(rows, n, kind, seed):
    """test_gpu_sfs's cohort with sample 0 het, sample 1 hom-alt and sample 2 not called (where the kind can say so) at every row."""
    max_allele, missing = KINDS[kind]
    x, called = cohort(rows, 2 * n, max_allele, missing, seed=seed)
    x = x.copy()
    called = None if called is None else called.copy()
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0, 1, 1, 1
    if called is not None:
        called[:, :4] = True
        called[:, 4] = False
    elif max_allele > 1:
        x[:, 5] = max_allele
    return x, called


def check_marked(dev, dm, x, called, kind, what, **kw):
    rows = x.shape[0]
    het, alt = qc_ref.sample_tables(x, called)[1:]
    assert het[0] == rows and alt[1] == rows and sum(t[2] for t in qc_ref.sample_tables(x, called)) == (rows if kind == "complete" else 0)
    got = check(dev, dm, x, called, what, weights=row_weights(rows, 1), **kw)
    assert got.sample["het"][0] == rows and got.sample["hom_alt"][1] == rows, what
    return got


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_row_count(dev, kind):
    max_allele, _ = KINDS[kind]
    for rows in ROWS:
        x, called = marked_cohort(rows, 34, kind, seed=6)
        if rows >= 64:
            preconditions(kind, x, called)
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            check_marked(dev, dm, x, called, kind, (kind, rows))
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["complete", "multi3-missing"])
def test_rows_around_the_counter_capacity(dev, fmh_opts, kind):
    """A lane's slices are emptied after 31 blocks of 8 rows = 248 of ITS rows: 7 936 rows of an item at 34 samples (32 row lanes), 248 at
    2 100 samples (one row lane).  One row less, that many, one more, and twice that many plus one (two expansions and a remainder)."""
    max_allele, _ = KINDS[kind]
    for n, edge in ((34, 7936), (2100, 248)):
        for rows in (edge - 1, edge, edge + 1, 2 * edge + 1):
            x, called = marked_cohort(rows, n, kind, seed=7)
            dm = upload(dev, x, called, max_allele, True, ploidy=2)
            try:
                fmh_opts.setenv("FMH_QC_ITEM_ROWS", str(1 << 20))  # one item holds every row
                long_item = check_marked(dev, dm, x, called, kind, (kind, n, rows, "one item"))
                fmh_opts.reset()
                default = check_marked(dev, dm, x, called, kind, (kind, n, rows, "default items"))
                for name in CLASSES:
                    assert np.array_equal(long_item.sample[name], default.sample[name])
            finally:
                dm.close()


# ---- options: several items per workgroup, several workgroups adding into the same sample slots ------------------------------------------------
@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_item_rows_and_grids_change_nothing(dev, fmh_opts, kind):
    max_allele, missing = KINDS[kind]
    for n, rows, settings in ((70, 1300, [(i, b) for i in (1, 8, 100) for b in (1, 2, 3)]), (4100, 300, [(100, 2), (8, 3)])):
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=8)
        weights = row_weights(rows)
        preconditions(kind, x, called, None, weights)
        keep = np.random.default_rng(rows).random(rows) < 0.5
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            for item_rows, blocks in settings:
                fmh_opts.setenv("FMH_QC_ITEM_ROWS", str(item_rows))
                fmh_opts.setenv("FMH_GRID_BLOCKS", str(blocks))
                check(dev, dm, x, called, (kind, n, item_rows, blocks), weights=weights)
                check(dev, dm, x, called, (kind, n, item_rows, blocks, "half"), weights=weights, keep=keep)
            fmh_opts.reset()
            fmh_opts.setenv("FMH_GRID_PER_CU", "1")
            check(dev, dm, x, called, (kind, n, "one workgroup per CU"), weights=weights, keep=keep)
            fmh_opts.reset()
        finally:
            dm.close()


# ---- call arguments ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_sample_lists(dev, kind):
    max_allele, missing = KINDS[kind]
    rng = np.random.default_rng(7)
    for total, rows in ((3, 300), (68, 300), (260, 300), (4100, 70)):
        x, called = cohort(rows, 2 * total, max_allele, missing, seed=26)
        weights = row_weights(rows)
        dm = upload(dev, x, called, max_allele, True, ploidy=2)
        try:
            gaps = np.flatnonzero(rng.random(total) < 0.6)
            if gaps.size == 0:
                gaps = np.array([total - 1])
            lists = {"none": None, "identity": np.arange(total), "gaps": gaps, "last-two": np.arange(max(total - 2, 0), total)}
            for name, samples in lists.items():
                if total >= 68 and name != "last-two":
                    preconditions(kind, x, called, samples, weights)
                check(dev, dm, x, called, (kind, total, name), samples=samples, weights=weights)
            if total == 68:
                check(dev, dm, x, called, (kind, total, "first 65"), n_samples=65, weights=weights)
        finally:
            dm.close()


def keep_masks(rows, seed):
    """all, none, one row, alternating, first half, random, only the last row"""
    rng = np.random.default_rng(rows + seed)
    one, last = np.zeros(rows, dtype=bool), np.zeros(rows, dtype=bool)
    one[rows // 3] = True
    last[-1] = True
    return {"all": np.ones(rows, dtype=bool), "none": np.zeros(rows, dtype=bool), "one": one, "alternating": np.arange(rows) % 2 == 0,
            "first-half": np.arange(rows) < rows // 2, "random": rng.random(rows) < 0.5, "last": last}


@pytest.mark.parametrize("kind", list(KINDS))
def test_row_ranges_and_keep_masks(dev, kind):
    max_allele, missing = KINDS[kind]
    n = 40
    for rows in (9, 300, 1300):
        x, called = cohort(rows, 2 * n, max_allele, missing, seed=9)
        weights = row_weights(rows)
        dm = upload(dev, x, called, max_allele, rows % 2 == 0, ploidy=2)
        try:
            for name, keep in keep_masks(rows, 3).items():
                got = check(dev, dm, x, called, (kind, rows, name), keep=keep, weights=weights)
                if name == "none":
                    assert got.kept_rows == 0 and not any(t.any() for t in got.sample.values())
            r0, rc = rows // 3, rows - rows // 3 - 1
            check(dev, dm, x, called, (kind, rows, "range"), row_begin=r0, row_count=rc, weights=weights[:rc])
            check(dev, dm, x, called, (kind, rows, "range+mask"), row_begin=r0, row_count=rc, keep=keep_masks(rc, 4)["random"], weights=weights[:rc])
            check(dev, dm, x, called, (kind, rows, "last row"), row_begin=rows - 1, row_count=1, weights=weights[:1])
        finally:
            dm.close()


@pytest.mark.parametrize("kind", ["complete", "missing", "multi7"])
def test_adds_accumulates_and_repeats_on_a_stream(dev, kind):
    import torch

    max_allele, missing = KINDS[kind]
    n = 70
    xa, ca = cohort(300, 2 * n, max_allele, missing, seed=10)
    xb, cb = cohort(513, 2 * n, max_allele, missing, seed=11)
    wa, wb = row_weights(300), row_weights(513, 2)
    preconditions(kind, xa, ca, None, wa)
    ma, mb = upload(dev, xa, ca, max_allele, True, ploidy=2), upload(dev, xb, cb, max_allele, False, ploidy=2)
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    names = CLASSES + ("weighted_called",)
    try:
        # buffers that are not zero beforehand: the call adds
        fill = np.arange(n, dtype=np.uint64) * np.uint64(1 << 40) + np.uint64(5)
        bufs = dev.GenotypeSampleBuffers(ma.device, n, names, fill=fill)
        got = dev.genotype_counts(ma, weights=wa, into=bufs, stream=handle)
        ref_a = dict(zip(names, qc_ref.sample_tables(xa, ca) + (qc_ref.weighted_called(xa, ca, wa),)))
        for name in names:
            assert np.array_equal(got.sample[name], ref_a[name] + fill), name
        # two matrices of the same samples accumulate: the oracle on their concatenation
        bufs = dev.GenotypeSampleBuffers(ma.device, n, names)
        dev.genotype_counts(ma, weights=wa, into=bufs, stream=handle)
        got = dev.genotype_counts(mb, weights=wb, into=bufs, stream=handle)
        xc, cc, wc = np.concatenate([xa, xb]), None if ca is None else np.concatenate([ca, cb]), np.concatenate([wa, wb])
        ref = dict(zip(names, qc_ref.sample_tables(xc, cc) + (qc_ref.weighted_called(xc, cc, wc),)))
        for name in names:
            assert np.array_equal(got.sample[name], ref[name]), name
        for name, r in zip(CLASSES, qc_ref.site_tracks(xb, cb)):   # the tracks are written, and are the second matrix's
            assert np.array_equal(got.site[name], r), name
        # the same input twice: the same bits
        again = dev.genotype_counts(mb, weights=wb, stream=handle)
        once = dev.genotype_counts(mb, weights=wb)
        for name in names:
            assert np.array_equal(again.sample[name], once.sample[name]), name
        for name in CLASSES:
            assert np.array_equal(again.site[name], once.site[name]), name
        stream.synchronize()
    finally:
        ma.close()
        mb.close()


def test_every_null_output_combination(dev):
    x, called = cohort(300, 140, 3, True, seed=13)
    weights = row_weights(300)
    keep = np.arange(300) % 3 != 0
    dm = upload(dev, x, called, 3, True, ploidy=2)
    site_ref = dict(zip(CLASSES, qc_ref.site_tracks(x, called)))
    sample_ref = dict(zip(CLASSES, qc_ref.sample_tables(x, called, None, keep)))
    weighted_ref = qc_ref.weighted_called(x, called, weights, None, keep)
    subsets = [(), ("hom_ref",), ("het",), ("hom_alt",), ("hom_ref", "hom_alt"), CLASSES]
    try:
        for site in subsets:
            for sample in subsets:
                for w in (None, weights):
                    if not site and not sample and w is None:
                        continue
                    got = dev.genotype_counts(dm, keep=keep, weights=w, site=site, sample=sample, fill=0x5A)
                    assert (got.site is None) == (not site) and sorted(got.site or ()) == sorted(site)
                    for name in site:
                        assert np.array_equal(got.site[name], site_ref[name]), (site, sample, name)
                    expect = set(sample) | ({"weighted_called"} if w is not None else set())
                    assert set(got.sample or ()) == expect
                    for name in sample:
                        assert np.array_equal(got.sample[name], sample_ref[name]), (site, sample, name)
                    if w is not None:
                        assert np.array_equal(got.sample["weighted_called"], weighted_ref), (site, sample)
                    assert got.kept_rows == 200
    finally:
        dm.close()


def test_refusals_leave_no_launch_error(dev):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, called = cohort(40, 16, 1, True, seed=12)
    dm = upload(dev, x, called, 1, True, ploidy=2)
    haploid = upload(dev, x, called, 1, True, ploidy=1)
    wide = cohort(40, 16, 1, False, seed=12)[0].copy()
    wide[0, 0] = 9  # an allele >= 8: u8 rows only, no packed image
    unpacked = dev.DeviceMatrix.from_host(wide, None, 40, 8, 2, 9)
    names = CLASSES + ("weighted_called",)
    bufs = dev.GenotypeSampleBuffers(dm.device, 8, names)
    tracks = [dev.DeviceBuffer(dm.device, 160) for _ in range(3)]
    site = _abi.GenotypeSiteOut(*[t.ptr for t in tracks])
    no_weighted = _abi.GenotypeSampleOut(*[bufs.bufs[k].ptr for k in CLASSES], None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    weights = row_weights(40)

    def call(m=dm, samples=None, n=8, r0=0, rc=40, k=None, w=None, s=site, t=no_weighted):
        return lib.fmh_genotype_counts(m._h if m is not None else None, None if samples is None else p(samples), n, r0, rc, None if k is None else p(k),
                                       None if w is None else p(w), None if s is None else C.byref(s), None if t is None else C.byref(t), None, None)

    try:
        assert call() == 0
        invalid = [call(m=None), call(n=0), call(n=9), call(samples=u32(0, 8), n=2), call(samples=u32(3, 3), n=2), call(samples=u32(4, 2), n=2),
                   call(r0=41, rc=0), call(r0=1, rc=40), call(r0=0, rc=41), call(s=None, t=None),
                   call(s=_abi.GenotypeSiteOut(None, None, None), t=_abi.GenotypeSampleOut(None, None, None, None)),
                   call(w=weights), call(w=weights, t=None), call(t=bufs.out), call(s=None, t=_abi.GenotypeSampleOut(None, None, None, bufs.bufs["weighted_called"].ptr))]
        assert invalid == [_abi.FMH_ERR_INVALID] * len(invalid), invalid
        assert call(m=haploid, n=4) == _abi.FMH_ERR_UNSUPPORTED and b"ploidy" in lib.fmh_last_error()
        assert call(m=unpacked) == _abi.FMH_ERR_UNSUPPORTED and b"fmh_matrix_pack" in lib.fmh_last_error()
        # nothing was added by a refused call, no launch error is left behind, and a keep mask of nothing adds nothing
        assert call(k=np.zeros(40, dtype=np.uint8), w=weights, t=bufs.out) == 0
        tables = bufs.tables()
        for name, ref in zip(CLASSES, qc_ref.sample_tables(x, called)):
            assert np.array_equal(tables[name], ref), name
        assert not tables["weighted_called"].any()
        check(dev, dm, x, called, "after the refusals", weights=weights)
        assert lib.fmh_hwe_exact(None, None, None, 0, None, dm.device, None) == 0
        assert lib.fmh_hwe_exact(tracks[0].ptr, None, tracks[2].ptr, 40, tracks[1].ptr, dm.device, None) == _abi.FMH_ERR_INVALID
    finally:
        dm.close()
        haploid.close()
        unpacked.close()


# ---- against an algebra that shares nothing: the diagonals of kinship's Grams ----------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_tables_equal_the_diagonals_of_kinship(dev, kind):
    max_allele, missing = KINDS[kind]
    x, called = cohort(600, 2 * 90, max_allele, missing, seed=14)
    preconditions(kind, x, called)
    keep = np.random.default_rng(14).random(600) < 0.7
    samples = np.flatnonzero(np.random.default_rng(15).random(90) < 0.8)
    dm = upload(dev, x, called, max_allele, True, ploidy=2)
    try:
        kin = dev.kinship_counts(dm, samples=samples, keep=keep)
        got = dev.genotype_counts(dm, samples=samples, keep=keep, site=())
        called_count = got.sample["hom_ref"] + got.sample["het"] + got.sample["hom_alt"]
        assert np.array_equal(np.diag(kin.both), called_count)
        assert np.array_equal(np.diag(kin.het_het), got.sample["het"])
        assert np.array_equal(np.diag(kinship_ref.tables(x, called, samples, keep)[0]), called_count)
    finally:
        dm.close()


# ---- the exact test on the device ---------------------------------------------------------------------------------------------------------------
def assert_bitwise(got, ref, what):
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    assert np.array_equal(got.view(np.uint64)[ok], ref.view(np.uint64)[ok]), (what, np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))[:4].tolist())


def test_hwe_device_is_the_host_twin_and_the_python_loop(dev):
    from tests.test_qc_cpu import SPECIAL, all_triples

    # short and long walks in adjacent lanes: N = 2 500 near the mode next to rare = 1, and the two underflows
    mixed = np.array([(625, 1250, 625), (9, 1, 0), (600, 1300, 600), (0, 1, 2499), (1250, 0, 1250), (1, 1, 0), (0, 2500, 0), (2499, 1, 0)] * 40, dtype=np.uint32)
    beyond = np.array([((1 << 26) + 1, 0, 0), (1 << 26, 0, 0)], dtype=np.uint32)   # N > 2^26: NaN from the device
    for name, t in (("N <= 12", all_triples(12)), ("special", SPECIAL), ("mixed", mixed)):
        got = dev.hwe_exact(0, t[:, 0], t[:, 1], t[:, 2])
        assert_bitwise(got, dev.hwe_exact_host(t[:, 0], t[:, 1], t[:, 2]), name + " against the host twin")
        assert_bitwise(got, qc_ref.hwe(t[:, 0], t[:, 1], t[:, 2]), name + " against the Python loop")
    got = dev.hwe_exact(0, beyond[:, 0], beyond[:, 1], beyond[:, 2])
    assert np.isnan(got[0]) and got[1] == 1.0
    zero = dev.hwe_exact(0, SPECIAL[10:, 0], SPECIAL[10:, 1], SPECIAL[10:, 2])
    assert not zero.view(np.uint64).any(), "exactly +0.0"


# ---- through `import ferromic` --------------------------------------------------------------------------------------------------------------------
def assert_qc(qc, x, called, samples, keep, what, hwe=True, inbreeding=True):
    n = x.shape[1] // 2 if samples is None else len(samples)
    site = qc_ref.site_tracks(x, called, samples)
    for name, r in zip(CLASSES, site):
        g = getattr(qc, name)
        assert g.dtype == np.uint32 and np.array_equal(g, r), (what, name)
    stats = qc_ref.site_stats(*site, n)
    for name in ("call_rate", "alt_frequency", "maf", "f_is"):
        assert_bitwise(getattr(qc, name), stats[name], (what, name))
    if hwe:
        assert_bitwise(qc.hwe_p, qc_ref.hwe(*site), (what, "hwe_p"))
    else:
        assert qc.hwe_p is None
    table = qc_ref.sample_tables(x, called, samples, keep)
    for name, r in zip(CLASSES, table):
        g = getattr(qc, "sample_" + name)
        assert g.dtype == np.uint64 and np.array_equal(g, r), (what, "sample", name)
    kept = x.shape[0] if keep is None else int(np.count_nonzero(keep))
    assert qc.kept_rows == kept
    weighted = qc_ref.weighted_called(x, called, qc_ref.site_weights(*site), samples, keep) if inbreeding else None
    sstats = qc_ref.sample_stats(*table, kept, weighted)
    assert_bitwise(qc.sample_call_rate, sstats["call_rate"], (what, "sample_call_rate"))
    assert_bitwise(qc.sample_het_rate, sstats["het_rate"], (what, "sample_het_rate"))
    if inbreeding:
        assert np.array_equal(qc.sample_weighted_called, weighted), what
        assert_bitwise(qc.sample_f, sstats["f"], (what, "sample_f"))
    else:
        assert qc.sample_f is None and qc.sample_weighted_called is None
    assert np.array_equal(qc.samples, np.arange(x.shape[1] // 2) if samples is None else np.asarray(samples)), what


def test_population_from_numpy(fm):
    """300 sites x 40 diploid samples with missing calls; the population holds both haplotypes of 22 samples and one of three more."""
    rng = np.random.default_rng(41)
    x, called = cohort(300, 80, 1, True, seed=41)
    geno = np.where(called, x, -1).astype(np.int8).reshape(300, 40, 2)
    whole = sorted(int(s) for s in rng.choice(40, size=22, replace=False))
    preconditions("missing", x, called, whole)
    halves = [s for s in range(40) if s not in whole][:3]
    haps = [(s, side) for s in whole for side in (0, 1)] + [(s, 1) for s in halves]
    pop = fm.Population.from_numpy("p", geno, np.arange(300, dtype=np.int64) * 7, haps, 3000)
    qc = pop.genotype_qc()
    assert isinstance(qc, fm.GenotypeQC)
    assert_qc(qc, x, called, whole, None, "Population.genotype_qc")
    assert_qc(pop.genotype_qc(hwe=False, inbreeding=False), x, called, whole, None, "without hwe and F", hwe=False, inbreeding=False)
    # `sites` restricts the sample arrays and the weights, never the site arrays
    sites = qc.site_filter(min_call_rate=0.95, min_maf=0.02, min_hwe_p=1e-6)
    assert sites.dtype == bool and sites.shape == (300,) and 0 < sites.sum() < 300
    restricted = pop.genotype_qc(sites=sites)
    assert_qc(restricted, x, called, whole, sites, "Population.genotype_qc(sites)")
    assert (restricted.sample_het != qc.sample_het).any() and np.array_equal(restricted.het, qc.het)
    # the filter plugs straight into kinship
    k = pop.kinship(sites=sites)
    assert np.array_equal(k.sites, np.flatnonzero(sites))
    assert np.array_equal(np.diag(k.both), restricted.sample_hom_ref + restricted.sample_het + restricted.sample_hom_alt)
    assert np.array_equal(np.diag(k.het_het), restricted.sample_het)
    keep = qc.sample_filter(min_call_rate=0.9, max_abs_f=0.5)
    assert keep.dtype == bool and keep.shape == (22,)
    with pytest.raises(ValueError):
        pop.genotype_qc(sites=np.ones(299, dtype=bool))
    with pytest.raises(ValueError):
        pop.genotype_qc(hwe=False).site_filter(min_hwe_p=0.1)


def test_genotype_qc_of_variant_records(fm):
    """A sparse variant list (records with missing genotypes), a region that cuts rows off both ends, a sample list, a sites mask."""
    x, called = cohort(60, 24, 1, True, seed=24)
    variants = []
    for i in range(60):
        calls = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(12)]
        variants.append(dict(position=100 + 10 * i, genotypes=calls))
    eff_called = np.repeat(called[:, 0::2], 2, axis=1)
    assert_qc(fm.genotype_qc(variants), x, eff_called, None, None, "genotype_qc")
    samples = [1, 2, 5, 10, 11]
    assert_qc(fm.genotype_qc(variants, samples=samples), x, eff_called, samples, None, "genotype_qc(samples)")
    region = (155, 612)  # positions 160 .. 610: rows 6 .. 51
    assert_qc(fm.genotype_qc(variants, region=region), x[6:52], eff_called[6:52], None, None, "genotype_qc(region)")
    sites = np.arange(46) % 3 != 1
    assert_qc(fm.genotype_qc(variants, samples=samples, sites=sites, region=region, hwe=False), x[6:52], eff_called[6:52], samples, sites,
              "genotype_qc(all arguments)", hwe=False)
    for bad in ([2, 1], [0, 0], [12], [-1]):
        with pytest.raises(ValueError):
            fm.genotype_qc(variants, samples=bad)
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s])] for s in range(12)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.genotype_qc(haploid)
