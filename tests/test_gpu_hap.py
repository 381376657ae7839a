"""Haplotype homozygosity windows on the device (fmh_haplotype_windows) against tests/hap_ref.py, the numpy oracle written from the
definition.  Every comparison is array_equal on integers: the window records, the canonical partition, and the same outputs again under
every launch shape (threads per workgroup, row tables on or off, windows asked for together or one call at a time, a grid smaller than the
window count).

Shapes are the smallest at which each part of the kernel can go wrong: a partial last dword and last 16-byte vector, one to five vectors,
windows of 0, 1, 2 and around 32 rows and one of 300, more members than a workgroup has threads (several members per thread), a partition
whose bitmap is longer than one wave's pass of the scan, the largest group the kernel takes, and more windows than the persistent grid has
workgroups.  Cohorts are those of tests/test_gpu_sfs.py (the bit-plane upload puts random bits under the uncalled entries) and crafted ones:
all members identical, all distinct early, classes that differ in one row, in calledness only, in an upper plane only, and planted class
sizes with ties."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import hap_ref
from tests.test_gpu_sfs import KINDS, cohort, upload

pytestmark = pytest.mark.gpu

COLUMNS = [1, 2, 63, 64, 65, 127, 128, 129, 257, 513]
# rows per window 0, 1, 2, 31, 32, 33, 300; overlapping, empty, unordered, the whole matrix, up to the last row
WINDOWS = [(0, 300), (7, 7), (0, 1), (5, 7), (100, 131), (0, 32), (267, 300), (299, 300), (3, 5), (300, 300), (90, 123)]


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


@pytest.fixture(scope="module")
def cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def group_masks(cols, seed):
    """all columns; a single member; members only in the last (partial) 16-byte vector; a random half; every second column"""
    rng = np.random.default_rng(cols + seed)
    one = np.zeros(cols, dtype=bool)
    one[cols // 3] = True
    last = np.zeros(cols, dtype=bool)
    first_of_last = (cols - 1) // 128 * 128
    last[first_of_last:] = rng.random(cols - first_of_last) < 0.6
    last[cols - 1] = True
    half = rng.random(cols) < 0.5
    half[rng.integers(cols)] = True
    second = np.zeros(cols, dtype=bool)
    second[(cols - 1) % 2::2] = True  # ends on the last column
    return {"all": np.ones(cols, dtype=bool), "one": one, "last-vector": last, "half": half, "every-second": second}


def run(dev, dm, mask, windows, partition=True, **kw):
    g = dev.Groups(dm, np.asarray(mask)[None, :].astype(np.uint8))
    try:
        return dev.haplotype_windows(dm, g, windows, partition=partition, **kw)
    finally:
        g.close()


def assert_equal(got, ref, what, partition=True):
    assert got.sum_sq.dtype == np.uint64 and got.distinct.dtype == np.uint32 and got.top.dtype == np.uint32, what
    assert np.array_equal(got.sum_sq, ref["sum_sq"]), what
    assert np.array_equal(got.distinct, ref["distinct"]), what
    assert np.array_equal(got.top, ref["top"]), what
    if partition:
        assert got.first.dtype == np.uint32 and np.array_equal(got.first, ref["first"]), what
    else:
        assert got.first is None, what


def same_outputs(a, b):
    return (np.array_equal(a.sum_sq, b.sum_sq) and np.array_equal(a.distinct, b.distinct) and np.array_equal(a.top, b.top)
            and (a.first is None) == (b.first is None) and (a.first is None or np.array_equal(a.first, b.first)))


def upload_crafted(dev, x, called, max_allele):
    return upload(dev, np.ascontiguousarray(x, dtype=np.uint8), called, max_allele, planes=True)


# ---- geometry x groups x matrix kinds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_geometry_and_group(dev, kind):
    max_allele, missing = KINDS[kind]
    rows = 300
    split_by_calledness = split_high = 0
    for cols in COLUMNS:
        x, called = cohort(rows, cols, max_allele, missing)
        dm = upload(dev, x, called, max_allele, planes=True)
        try:
            for name, mask in group_masks(cols, 3).items():
                ref = hap_ref.windows(x, called, mask, WINDOWS)
                got = run(dev, dm, mask, WINDOWS)
                assert_equal(got, ref, (kind, cols, name))
                n = int(mask.sum())
                assert (got.top.sum(axis=1) <= n).all() and (got.distinct >= 1).all()
                assert got.distinct[1] == 1 and got.sum_sq[1] == n * n and got.top[1].tolist() == [n, 0, 0]  # the empty window
                assert (got.first <= np.arange(n)[None, :]).all()
                # not vacuous (from the oracle): classes that only the called plane / an upper plane tells apart
                if missing:
                    split_by_calledness += int((hap_ref.windows(x, None, mask, WINDOWS)["distinct"] != ref["distinct"]).sum())
                if max_allele > 1:
                    split_high += int((hap_ref.windows(x & 1, called, mask, WINDOWS)["distinct"] != ref["distinct"]).sum())
        finally:
            dm.close()
    assert (split_by_calledness > 0) == missing and (split_high > 0) == (max_allele > 1)


@pytest.mark.parametrize("kind", ["missing", "multi7"])
def test_windows_together_and_one_per_call(dev, kind):
    max_allele, missing = KINDS[kind]
    rows, cols = 300, 257
    x, called = cohort(rows, cols, max_allele, missing, seed=11)
    mask = group_masks(cols, 11)["half"]
    ref = hap_ref.windows(x, called, mask, WINDOWS)
    dm = upload(dev, x, called, max_allele, planes=True)
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    try:
        together = dev.haplotype_windows(dm, g, WINDOWS, partition=True)
        assert_equal(together, ref, kind)
        for w, window in enumerate(WINDOWS):
            one = dev.haplotype_windows(dm, g, [window], partition=True)
            assert one.sum_sq[0] == together.sum_sq[w] and one.distinct[0] == together.distinct[w]
            assert np.array_equal(one.top[0], together.top[w]) and np.array_equal(one.first[0], together.first[w]), window
        whole = dev.haplotype_windows(dm, g)  # default: one window, every row; no partition
        assert_equal(whole, {k: v[:1] for k, v in ref.items()}, "default window", partition=False)
    finally:
        g.close()
        dm.close()


# ---- crafted cohorts --------------------------------------------------------------------------------------------------------------------
def test_all_members_identical(dev):
    """K stays 1 over every row: all members set the same bit of the same bitmap word at every step."""
    rows, cols = 40, 513
    rng = np.random.default_rng(1)
    x = np.repeat(rng.integers(0, 4, size=(rows, 1), dtype=np.uint8), cols, axis=1)
    called = np.repeat(rng.random((rows, 1)) < 0.8, cols, axis=1)
    windows = [(0, rows), (3, 9), (0, 0)]
    dm = upload_crafted(dev, x, called, 3)
    try:
        for mask in (np.ones(cols, dtype=bool), group_masks(cols, 5)["half"]):
            got = run(dev, dm, mask, windows)
            assert_equal(got, hap_ref.windows(x, called, mask, windows), "identical")
            n = int(mask.sum())
            assert got.distinct.tolist() == [1, 1, 1] and got.top[:, 0].tolist() == [n, n, n] and not got.first.any()
    finally:
        dm.close()


def test_all_members_distinct_early(dev):
    """The first 9 rows spell the member's column in binary: K reaches n there, the 31 rows after it change nothing."""
    rows, cols = 40, 300
    rng = np.random.default_rng(2)
    x = rng.integers(0, 2, size=(rows, cols), dtype=np.uint8)
    x[:9] = (np.arange(cols)[None, :] >> np.arange(9)[:, None]) & 1
    windows = [(0, rows), (0, 9), (0, 8), (1, 40)]
    dm = upload_crafted(dev, x, None, 1)
    try:
        mask = np.ones(cols, dtype=bool)
        got = run(dev, dm, mask, windows)
        assert_equal(got, hap_ref.windows(x, None, mask, windows), "distinct")
        assert got.distinct[:2].tolist() == [cols, cols] and got.distinct[2] == 256 and got.top[0].tolist() == [1, 1, 1]
        assert np.array_equal(got.first[0], np.arange(cols))
    finally:
        dm.close()


@pytest.mark.parametrize("where", ["last-row", "first-row"])
def test_two_classes_that_differ_in_one_row_of_the_window(dev, where):
    rows, cols = 64, 129
    rng = np.random.default_rng(3)
    x = np.repeat(rng.integers(0, 2, size=(rows, 1), dtype=np.uint8), cols, axis=1)
    odd = np.arange(cols) % 3 == 1
    begin, end = 10, 43  # 33 rows
    row = end - 1 if where == "last-row" else begin
    x[row, odd] ^= 1
    windows = [(begin, end), (begin + 1, end - 1), (begin, end - 1), (begin + 1, end)]
    dm = upload_crafted(dev, x, None, 1)
    try:
        mask = np.ones(cols, dtype=bool)
        got = run(dev, dm, mask, windows)
        assert_equal(got, hap_ref.windows(x, None, mask, windows), where)
        assert got.distinct.tolist() == ([2, 1, 1, 2] if where == "last-row" else [2, 1, 2, 1])
        assert got.top[0].tolist() == [cols - int(odd.sum()), int(odd.sum()), 0]
    finally:
        dm.close()


def test_members_that_differ_only_in_calledness(dev):
    """Allele 0 everywhere; in row 5 a third of the members is not called (and carries random bits in the allele plane)."""
    rows, cols = 12, 257
    x = np.zeros((rows, cols), dtype=np.uint8)
    called = np.ones((rows, cols), dtype=bool)
    gone = np.arange(cols) % 3 == 0
    called[5, gone] = False
    windows = [(0, rows), (0, 5), (5, 6), (6, rows)]
    dm = upload_crafted(dev, x, called, 1)
    try:
        mask = np.ones(cols, dtype=bool)
        got = run(dev, dm, mask, windows)
        assert_equal(got, hap_ref.windows(x, called, mask, windows), "calledness")
        assert got.distinct.tolist() == [2, 1, 2, 1] and got.top[0].tolist() == [cols - int(gone.sum()), int(gone.sum()), 0]
    finally:
        dm.close()


@pytest.mark.parametrize("pair", [(1, 3), (2, 6)], ids=["1-against-3", "2-against-6"])
def test_members_that_differ_only_in_an_upper_plane(dev, pair):
    low, high = pair
    rows, cols = 9, 129
    x = np.zeros((rows, cols), dtype=np.uint8)
    x[4] = low
    other = np.arange(cols) % 5 == 2
    x[4, other] = high
    windows = [(0, rows), (4, 5), (0, 4)]
    dm = upload_crafted(dev, x, None, 3 if high <= 3 else 7)
    try:
        mask = np.ones(cols, dtype=bool)
        got = run(dev, dm, mask, windows)
        assert_equal(got, hap_ref.windows(x, None, mask, windows), pair)
        assert got.distinct.tolist() == [2, 2, 1] and got.top[1].tolist() == [cols - int(other.sum()), int(other.sum()), 0]
    finally:
        dm.close()


def test_planted_class_sizes_with_ties(dev):
    """Classes of 6, 4, 4, 3, 3, 3 and 1 members spread over the columns: ties for the second and the third largest."""
    sizes = [6, 4, 4, 3, 3, 3, 1]
    rng = np.random.default_rng(4)
    class_of = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    n = len(class_of)
    cols = 2 * n + 1
    members = np.sort(rng.choice(cols, size=n, replace=False))
    rows = 20
    patterns = rng.integers(0, 2, size=(rows, len(sizes)), dtype=np.uint8)
    patterns[:3] = (np.arange(len(sizes))[None, :] >> np.arange(3)[:, None]) & 1  # the classes differ
    x = rng.integers(0, 2, size=(rows, cols), dtype=np.uint8)
    x[:, members] = patterns[:, class_of]
    mask = np.zeros(cols, dtype=bool)
    mask[members] = True
    dm = upload_crafted(dev, x, None, 1)
    try:
        got = run(dev, dm, mask, [(0, rows)])
        assert_equal(got, hap_ref.windows(x, None, mask, [(0, rows)]), "planted")
        assert got.distinct[0] == 7 and got.top[0].tolist() == [6, 4, 4] and got.sum_sq[0] == 36 + 16 + 16 + 27 + 1
        stats = dev.haplotype_stats(got.sum_sq, got.distinct, got.top, n)
        ref = hap_ref.stats(96, [6, 4, 4], n)
        assert all(float(stats[k][0]) == ref[k] for k in dev.HAP_STATS)
    finally:
        dm.close()


# ---- wide partitions --------------------------------------------------------------------------------------------------------------------
def test_a_bitmap_longer_than_one_pass_of_the_scan(dev, fmh_opts):
    """2 100 members at frequency 0.5 on 16 rows: every member is its own class after a dozen rows, the bitmap of 2 K bits is then 132 words -
    more than the 64 threads of the smallest workgroup, and more than one wave, scan in one go."""
    rows, cols = 16, 2100
    x = np.random.default_rng(5).integers(0, 2, size=(rows, cols), dtype=np.uint8)
    mask = np.ones(cols, dtype=bool)
    windows = [(0, rows), (0, 11), (4, 16)]
    ref = hap_ref.windows(x, None, mask, windows)
    assert ref["distinct"][0] > 1024
    dm = upload_crafted(dev, x, None, 1)
    try:
        for threads in (None,) + dev.HAP_THREADS:
            if threads is not None:
                fmh_opts.setenv("FMH_HAP_THREADS", threads)
            assert_equal(run(dev, dm, mask, windows), ref, threads)
    finally:
        dm.close()


@functools.lru_cache(maxsize=None)
def largest_cohort(cap):
    rows, cols = 24, cap + 1
    rng = np.random.default_rng(6)
    x = rng.integers(0, 2, size=(rows, cols), dtype=np.uint8)
    x[:, : cols // 2] = x[:, cols // 2: 2 * (cols // 2)]  # every haplotype of the first half has a twin in the second
    x[20, ::7] ^= 1
    x.setflags(write=False)
    return x


def test_the_largest_group_and_one_member_more(dev):
    from ferromic_amd import _abi

    cap = dev.haplotype_max_members()
    x = largest_cohort(cap)
    mask = np.ones(cap + 1, dtype=bool)
    mask[cap // 3] = False  # exactly `cap` members
    windows = [(0, 24), (0, 3), (20, 21)]
    ref = hap_ref.windows(x, None, mask, windows)
    assert ref["distinct"][0] > cap // 2 and ref["top"][0][0] >= 2
    dm = upload(dev, x, None, 1, planes=True, ploidy=1)
    try:
        assert_equal(run(dev, dm, mask, windows), ref, "cap")
        with pytest.raises(_abi.FerromicHipError) as err:
            run(dev, dm, np.ones(cap + 1, dtype=bool), windows)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and str(cap) in str(err.value)
    finally:
        dm.close()


# ---- grid and launch --------------------------------------------------------------------------------------------------------------------
GRID_ROWS, GRID_COLS = 6161, 257


@functools.lru_cache(maxsize=None)
def grid_case():
    x, called = cohort(GRID_ROWS, GRID_COLS, 3, True)
    mask = group_masks(GRID_COLS, 3)["half"]
    windows = [(r, r + 2) for r in range(GRID_ROWS - 1)]
    return x, called, mask, windows, hap_ref.windows(x, called, mask, windows)


def test_more_windows_than_the_grid_has_workgroups(dev, fmh_opts, cus):
    """6 160 two-row windows of about 128 members (64 threads, eight workgroups per CU): every workgroup resets its labels, K and both bitmaps
    for a second and a third window; then the same with a grid of three workgroups."""
    x, called, mask, windows, ref = grid_case()
    assert len(windows) > 3 * 8 * cus, f"{cus} CUs: {len(windows)} windows no longer give every workgroup three"
    assert len(set(ref["distinct"].tolist())) > 3
    dm = upload(dev, x, called, 3, planes=True)
    try:
        assert_equal(run(dev, dm, mask, windows), ref, "default grid")
        fmh_opts.setenv("FMH_GRID_BLOCKS", 3)
        assert_equal(run(dev, dm, mask, windows[:400]), {k: v[:400] for k, v in ref.items()}, "three workgroups")
    finally:
        dm.close()


@pytest.mark.parametrize("row_hi", ["0", "2", None], ids=["row_hi=0", "row_hi=2", "row_hi=default"])
@pytest.mark.parametrize("kind", ["multi3-missing", "multi7"])
def test_threads_and_row_tables_change_nothing(dev, fmh_opts, kind, row_hi):
    max_allele, missing = KINDS[kind]
    rows, cols = 300, 513
    x, called = cohort(rows, cols, max_allele, missing, seed=13)
    mask = group_masks(cols, 13)["half"]  # about 256 members: four per thread at 64 threads, none for most threads at 1 024
    ref = hap_ref.windows(x, called, mask, WINDOWS)
    if row_hi is not None:
        fmh_opts.setenv("FMH_ROW_HI", row_hi)  # read when the matrix is made
    dm = upload(dev, x, called, max_allele, planes=True)
    try:
        outputs = []
        for threads in (None,) + dev.HAP_THREADS:
            if threads is not None:
                fmh_opts.setenv("FMH_HAP_THREADS", threads)
            for per_cu in (None, 1):
                if per_cu is not None:
                    fmh_opts.setenv("FMH_GRID_PER_CU", per_cu)
                else:
                    fmh_opts.delenv("FMH_GRID_PER_CU")
                outputs.append(run(dev, dm, mask, WINDOWS))
                assert_equal(outputs[-1], ref, (kind, row_hi, threads, per_cu))
        assert all(same_outputs(outputs[0], o) for o in outputs[1:])
    finally:
        dm.close()


def test_on_a_stream_into_outputs_full_of_junk(dev):
    """The C call on a stream of the caller's, twice, into buffers filled with 0xFF bytes: every entry is written; then without d_first."""
    import torch

    from ferromic_amd import _abi

    lib = _abi.load()
    rows, cols = 300, 513
    x, called = cohort(rows, cols, 3, True)
    mask = group_masks(cols, 7)["half"]
    n = int(mask.sum())
    ref = hap_ref.windows(x, called, mask, WINDOWS)
    w = np.array(WINDOWS, dtype=np.uint64)
    dm = upload(dev, x, called, 3, planes=True)
    g = dev.Groups(dm, mask[None, :].astype(np.uint8))
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    assert handle.value, "a stream of its own, not the NULL stream"
    try:
        d_out = dev.DeviceBuffer.from_numpy(dm.device, np.full(24 * len(WINDOWS), 0xFF, dtype=np.uint8))
        d_first = dev.DeviceBuffer.from_numpy(dm.device, np.full(4 * n * len(WINDOWS), 0xFF, dtype=np.uint8))
        for call in ("first", "second"):
            _abi.check(lib.fmh_haplotype_windows(dm._h, g._h, w.ctypes.data_as(C.c_void_p), len(WINDOWS), d_out.ptr, d_first.ptr, handle))
            rec = d_out.to_numpy(np.uint8, 24 * len(WINDOWS)).view(dev.HAP_WINDOW_DTYPE)
            assert np.array_equal(rec["sum_sq"], ref["sum_sq"]) and np.array_equal(rec["distinct"], ref["distinct"]), call
            assert np.array_equal(rec["top"], ref["top"]), call
            assert np.array_equal(d_first.to_numpy(np.uint32, n * len(WINDOWS)).reshape(len(WINDOWS), n), ref["first"]), call
        for partition in (True, False):  # the wrapper's own pre-fill, on the NULL stream
            assert_equal(run(dev, dm, mask, WINDOWS, partition=partition, fill=0xA5), ref, partition, partition=partition)
    finally:
        stream.synchronize()
        g.close()
        dm.close()


# ---- refusals on a live matrix ----------------------------------------------------------------------------------------------------------
def test_refusals(dev, fmh_opts):
    from ferromic_amd import _abi

    lib = _abi.load()
    x, _ = cohort(17, 513, 1, False)
    everyone = np.ones((1, 513), dtype=np.uint8)
    dm = upload(dev, x, None, 1)
    other = upload(dev, cohort(17, 65, 1, False)[0], None, 1)
    g = dev.Groups(dm, everyone)
    two = dev.Groups(dm, np.concatenate([everyone, everyone]))
    nobody = dev.Groups(dm, np.zeros((1, 513), dtype=np.uint8))
    foreign = dev.Groups(other, np.ones((1, 65), dtype=np.uint8))
    try:
        def refused(call, status, text):
            with pytest.raises(_abi.FerromicHipError) as err:
                call()
            assert err.value.status == status and text in str(err.value), str(err.value)

        refused(lambda: dev.haplotype_windows(dm, two), _abi.FMH_ERR_INVALID, "exactly 1 group")
        refused(lambda: dev.haplotype_windows(dm, foreign), _abi.FMH_ERR_INVALID, "not made for this matrix")
        refused(lambda: dev.haplotype_windows(dm, nobody), _abi.FMH_ERR_INVALID, "no member")
        refused(lambda: dev.haplotype_windows(dm, g, [(0, 17), (3, 18)]), _abi.FMH_ERR_INVALID, "exceed")  # past the end
        refused(lambda: dev.haplotype_windows(dm, g, [(9, 3)]), _abi.FMH_ERR_INVALID, "exceed")          # begin > end
        refused(lambda: dev.haplotype_windows(dm, g, np.zeros((0, 2), dtype=np.uint64)), _abi.FMH_ERR_INVALID, "n_windows")
        # the order: a wrong group count is found before a window outside the matrix, that before n_windows == 0
        refused(lambda: dev.haplotype_windows(dm, two, [(0, 99)]), _abi.FMH_ERR_INVALID, "exactly 1 group")
        # an oversize partition, asked for with many (empty) windows: refused before anything of that size exists
        n_windows = (1 << 32) // 513 + 1
        windows = np.zeros((n_windows, 2), dtype=np.uint64)
        small = dev.DeviceBuffer(dm.device, 64)
        status = lib.fmh_haplotype_windows(dm._h, g._h, windows.ctypes.data_as(C.c_void_p), n_windows, small.ptr, small.ptr, None)
        assert status == _abi.FMH_ERR_UNSUPPORTED and b"2^32" in lib.fmh_last_error()
        assert lib.fmh_haplotype_windows(dm._h, g._h, windows.ctypes.data_as(C.c_void_p), n_windows, None, small.ptr, None) == _abi.FMH_ERR_INVALID
    finally:
        for h in (g, two, nobody, foreign, dm, other):
            h.close()
    fmh_opts.setenv("FMH_LAYOUT", "bytes")  # the matrix keeps its u8 rows and gets no packed image
    dm = upload(dev, x, None, 1)
    g = dev.Groups(dm, everyone)
    try:
        with pytest.raises(_abi.FerromicHipError) as err:
            dev.haplotype_windows(dm, g)
        assert err.value.status == _abi.FMH_ERR_UNSUPPORTED and "fmh_matrix_pack" in str(err.value)
        dm.pack()
        assert_equal(dev.haplotype_windows(dm, g, partition=True), hap_ref.windows(x, None, np.ones(513, dtype=bool), [(0, 17)]), "after fmh_matrix_pack")
    finally:
        g.close()
        dm.close()


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------
def python_cohort():
    """40 sites x 6 diploid samples as variant records: site 5 carries an allele 2, site 9 has a sample without a genotype."""
    rng = np.random.default_rng(77)
    sites, samples = 40, 6
    x = (rng.random((sites, samples * 2)) < rng.beta(0.5, 1.2, size=sites)[:, None]).astype(np.uint8)
    x[5, 3] = 2
    called = np.ones(x.shape, dtype=bool)
    called[9, 4:6] = False
    positions = 100 + 10 * np.arange(sites)
    records = []
    for i in range(sites):
        genotypes = [None if not called[i, 2 * s] else [int(x[i, 2 * s]), int(x[i, 2 * s + 1])] for s in range(samples)]
        records.append(dict(position=int(positions[i]), genotypes=genotypes))
    return x, called, positions, records


def assert_python_equal(got, ref, n, ranges, partition):
    assert got.sample_size == n and len(got) == len(ranges)
    assert got.windows.tolist() == [list(r) for r in ranges]
    assert np.array_equal(got.sum_squares, ref["sum_sq"]) and np.array_equal(got.distinct, ref["distinct"]) and np.array_equal(got.top_counts, ref["top"])
    if partition:
        assert np.array_equal(got.first_identical, ref["first"])
    else:
        assert got.first_identical is None
    for w in range(len(ranges)):
        want = hap_ref.stats(ref["sum_sq"][w], ref["top"][w], n)
        for key, value in want.items():
            assert float(getattr(got, key)[w]) == value, (key, w)


def test_python_garud_h_of_variant_records(fm):
    x, called, positions, records = python_cohort()
    haps = [(0, 0), (0, 1), (2, 0), (2, 1), (3, 1), (5, 0)]
    mask = np.zeros(12, dtype=bool)
    for s, side in haps:
        mask[2 * s + side] = True
    every = [(s, side) for s in range(6) for side in (0, 1)]
    assert_python_equal(fm.garud_h(records, haps), hap_ref.windows(x, called, mask, [(0, 40)]), 6, [(0, 40)], False)
    assert_python_equal(fm.garud_h(records, every, partition=True), hap_ref.windows(x, called, np.ones(12, dtype=bool), [(0, 40)]), 12, [(0, 40)], True)
    # size / step in variants; the partial last window is dropped
    ranges = [(0, 7), (7, 14), (14, 21), (21, 28), (28, 35)]
    assert_python_equal(fm.garud_h(records, every, size=7, partition=True), hap_ref.windows(x, called, np.ones(12, dtype=bool), ranges), 12, ranges, True)
    ranges = [(i * 3, i * 3 + 10) for i in range(11)]  # 30 + 10 = 40 fits, 33 + 10 does not
    assert_python_equal(fm.garud_h(records, haps, size=10, step=3), hap_ref.windows(x, called, mask, ranges), 6, ranges, False)
    # region = positions 150..300 inclusive = rows 5..20; windows in rows of the region
    ranges = [(0, 4), (4, 8), (8, 12), (12, 16)]
    got = fm.garud_h(records, every, region=(150, 300), size=4, partition=True)
    assert_python_equal(got, hap_ref.windows(x[5:21], called[5:21], np.ones(12, dtype=bool), ranges), 12, ranges, True)
    # position windows: (start, end) inclusive, mapped to rows as the spectra's; a window without a variant is empty
    windows = [(100, 190), (400, 10**6), (0, 50), (180, 230), (95, 1000)]
    ranges = [(0, 10), (30, 40), (0, 0), (8, 14), (0, 40)]
    assert_python_equal(fm.garud_h(records, haps, windows=windows, partition=True), hap_ref.windows(x, called, mask, ranges), 6, ranges, True)
    # positions that do not ascend: a window of two runs of rows is refused, one that is a single run is not
    shuffled = records[20:] + records[:20]
    with pytest.raises(ValueError, match="more than one run"):
        fm.garud_h(shuffled, haps, windows=[(150, 350)])
    got = fm.garud_h(shuffled, haps, windows=[(310, 350)])  # rows 21..25 of the original = rows 1..5 of the shuffled list
    assert got.windows.tolist() == [[1, 6]] and np.array_equal(got.sum_squares, hap_ref.windows(x, called, mask, [(21, 26)])["sum_sq"])


def test_python_population_garud_h(fm):
    x, called, positions, records = python_cohort()
    dense = np.where(called, x, -1).astype(np.int8).reshape(40, 6, 2)
    h1 = [(s, side) for s in (0, 1, 2) for side in (0, 1)]
    h2 = [(s, side) for s in (2, 3, 4, 5) for side in (0, 1)][1:]
    m1, m2 = np.zeros(12, dtype=bool), np.zeros(12, dtype=bool)
    for s, side in h1:
        m1[2 * s + side] = True
    for s, side in h2:
        m2[2 * s + side] = True
    for make in (lambda h: fm.Population.from_numpy("d", dense, positions.astype(np.int64), h, 1000), lambda h: fm.Population("s", records, h, 1000)):
        base = make(h1 + h2)
        p1, p2 = base.with_haplotypes(0, h1), base.with_haplotypes(1, h2)
        assert_python_equal(p1.garud_h(), hap_ref.windows(x, called, m1, [(0, 40)]), 6, [(0, 40)], False)
        ranges = [(0, 20), (20, 40)]
        assert_python_equal(p2.garud_h(windows=[(100, 290), (300, 1000)], partition=True), hap_ref.windows(x, called, m2, ranges), 7, ranges, True)
        ranges = [(0, 16), (8, 24), (16, 32), (24, 40)]
        assert_python_equal(p2.garud_h(size=16, step=8, partition=True), hap_ref.windows(x, called, m2, ranges), 7, ranges, True)
