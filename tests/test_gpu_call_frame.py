"""What the device statistics' host entry points share, pinned over the C-ABI: the text and the order of the refusals several of them word
alike (rows past the end, a window or block past the end, a sample list out of range or not ascending, n_samples above the matrix's, a matrix
without its packed image), and what a call adds to the library's kernel time (fmh_timing_read) while fmh_timing_enable is on.  The texts and
the counts are copied from the sources: one timed span per call, one per chunk of fmh_ld_prune_chunked, none for fmh_kinship_counts, whose
stage timer reports through fmh_timing_read_gram alone.

One 16-variant by 8-sample diploid matrix, biallelic with nothing missing, as a packed handle and as a handle that holds u8 rows only (it
declares an allele above 7, which no bit plane holds)."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, N, COLS = 16, 8, 16
PAST = "rows [1, 17) exceed the matrix's 16 variants"
UNPACKED = " the bit-packed image: call fmh_matrix_pack first (the matrix holds u8 rows only)"
SAMPLE_RANGE = "sample 8 (entry 1) is outside the matrix's 8 samples"
SAMPLE_ORDER = "the sample list is not strictly ascending at entry 1"
SAMPLE_COUNT = "n_samples 9 exceeds the matrix's 8 samples"


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def u32(*v):
    return np.array(v, dtype=np.uint32)


def spans(*v):
    return np.array(v, dtype=np.uint64).reshape(-1, 2)


@pytest.fixture(scope="module")
def frame():
    """The two handles, groups, output buffers and one closure per entry point whose defaults make a valid call."""
    from ferromic_amd import _abi, device as dev

    lib = _abi.load()
    data = (np.random.default_rng(5).random((V, COLS)) < 0.4).astype(np.uint8)
    packed = dev.DeviceMatrix.from_host(data, None, V, N, 2, 1)
    wide = data.copy()
    wide[0, 0] = 9
    bytes_only = dev.DeviceMatrix.from_host(wide, None, V, N, 2, 9)
    everyone = np.ones((1, COLS), dtype=np.uint8)
    halves = np.zeros((2, COLS), dtype=np.uint8)
    halves[0, :8] = halves[1, 8:] = 1
    g1, g2 = dev.Groups(packed, everyone), dev.Groups(packed, halves)  # (of 16 columns on this device: they suit both handles)
    out = dev.DeviceBuffer(packed.device, 1 << 16)                    # every call's output fits; nothing reads it back
    tracks = [dev.DeviceBuffer(packed.device, V * 4) for _ in range(3)]
    site = _abi.GenotypeSiteOut(*[t.ptr for t in tracks])
    tables = _abi.KinshipOut(*[out.ptr + i * N * N * 8 for i in range(4)])
    band = _abi.LdBandOut(out.ptr, None, None, None)
    params = _abi.EhhParams(0, 1, 0, 0, 0, 0)
    two_windows, focal = spans((0, 8), (8, 16)), np.array([4, 9], dtype=np.uint64)
    values = np.arange(1, 2 * N + 1, dtype=np.int32)  # one column; more entries than any n_samples a call below declares
    keep = np.zeros(V, dtype=np.uint8)
    h = lambda m: m._h

    def hap(m=packed, windows=two_windows, d_out=out.ptr):
        return lib.fmh_haplotype_windows(h(m), g1._h, p(windows), len(windows), d_out, None, None)

    def ehh(m=packed, r0=0, r1=V, d_out=out.ptr):
        return lib.fmh_ehh_scan(h(m), g1._h, r0, r1, p(focal), 2, None, C.byref(params), d_out, None, None)

    def sfs(m=packed, windows=two_windows, d_sfs=out.ptr):
        return lib.fmh_sfs(h(m), g1._h, p(windows), len(windows), d_sfs, None, None)

    def sfs_joint(m=packed, r0=0, rc=V, d_sfs=out.ptr):
        return lib.fmh_sfs_joint(h(m), g2._h, r0, rc, d_sfs, None, None)

    def fstat(m=packed, blocks=two_windows, d_moments=out.ptr):
        return lib.fmh_fstat_moments(h(m), p(halves), 2, p(blocks), len(blocks), d_moments, None, None)

    def qc(m=packed, samples=None, n=N, r0=0, rc=V, s=site):
        return lib.fmh_genotype_counts(h(m), p(samples), n, r0, rc, None, None, None if s is None else C.byref(s), None, None, None)

    def hwe():  # after qc(): the three tracks hold counts
        return lib.fmh_hwe_exact(tracks[0].ptr, tracks[1].ptr, tracks[2].ptr, V, out.ptr, packed.device, None)

    def assoc(m=packed, samples=None, n=N, r0=0, rc=V, d_sum=out.ptr):
        return lib.fmh_assoc_sums(h(m), p(samples), n, r0, rc, p(values), 1, d_sum, None, None)

    def ld_band(m=packed, r0=0, rc=V, end=V, d_out=band):
        return lib.fmh_ld_band(h(m), None, r0, rc, end, 4, 0.0, None if d_out is None else C.byref(d_out), None, None, None)

    def ld_prune(m=packed, r0=0, rc=V, h_keep=keep):
        return lib.fmh_ld_prune_chunked(h(m), None, r0, rc, 4, 0.5, p(h_keep), 8, None)  # 8 rows per chunk: two chunks

    def kinship(m=packed, samples=None, n=N, r0=0, rc=V, o=tables):
        return lib.fmh_kinship_counts(h(m), p(samples), n, r0, rc, None, None if o is None else C.byref(o), None, None)

    calls = dict(hap=hap, ehh=ehh, sfs=sfs, sfs_joint=sfs_joint, fstat=fstat, qc=qc, hwe=hwe, assoc=assoc, ld_band=ld_band, ld_prune=ld_prune,
                 kinship=kinship)
    yield lib, _abi, calls, bytes_only
    for handle in (g1, g2, packed, bytes_only):
        handle.close()


def refused(lib, status, want_status, want_text):
    text = lib.fmh_last_error().decode()
    print(status, text)
    assert (status, text) == (want_status, want_text)


def test_shared_refusals_keep_their_text(frame):
    lib, _abi, c, bytes_only = frame
    INVALID, UNSUPPORTED = _abi.FMH_ERR_INVALID, _abi.FMH_ERR_UNSUPPORTED
    second = spans((0, 8), (8, 17))
    # rows past the end
    refused(lib, c["ehh"](r1=17), INVALID, "rows [0, 17) exceed the matrix's 16 variants")
    refused(lib, c["ehh"](r0=5, r1=3), INVALID, "rows [5, 3) exceed the matrix's 16 variants")
    refused(lib, c["sfs_joint"](r0=1), INVALID, "rows [1, 17) of window 0 exceed the matrix's 16 variants")
    for name in ("qc", "assoc", "ld_prune", "kinship"):
        refused(lib, c[name](r0=1), INVALID, PAST)
    refused(lib, c["qc"](r0=17, rc=0), INVALID, "rows [17, 17) exceed the matrix's 16 variants")
    # entry 1 of a table past the end
    refused(lib, c["hap"](windows=second), INVALID, "rows [8, 17) of window 1 exceed the matrix's 16 variants")
    refused(lib, c["sfs"](windows=second), INVALID, "rows [8, 17) of window 1 exceed the matrix's 16 variants")
    refused(lib, c["fstat"](blocks=second), INVALID, "rows [8, 17) of block 1 exceed the matrix's 16 variants")
    refused(lib, c["fstat"](blocks=spans((0, 8), (9, 8))), INVALID, "rows [9, 8) of block 1 exceed the matrix's 16 variants")
    # the sample list and n_samples
    for name in ("qc", "assoc", "kinship"):
        refused(lib, c[name](samples=u32(0, 8), n=2), INVALID, SAMPLE_RANGE)
        refused(lib, c[name](samples=u32(3, 3), n=2), INVALID, SAMPLE_ORDER)
        refused(lib, c[name](samples=u32(4, 2), n=2), INVALID, SAMPLE_ORDER)
        refused(lib, c[name](n=9), INVALID, SAMPLE_COUNT)
    # u8 rows only
    for name, who in (("hap", "the haplotype windows read"), ("ehh", "the haplotype scan reads"), ("sfs", "the site frequency spectrum reads"),
                      ("sfs_joint", "the site frequency spectrum reads"), ("fstat", "the f-statistics read"), ("qc", "genotype QC reads"),
                      ("assoc", "the association scan reads"), ("ld_band", "linkage disequilibrium reads"),
                      ("ld_prune", "linkage disequilibrium reads"), ("kinship", "kinship reads")):
        refused(lib, c[name](m=bytes_only), UNSUPPORTED, who + UNPACKED)


def test_the_earlier_refusal_wins(frame):
    lib, _abi, c, bytes_only = frame
    INVALID = _abi.FMH_ERR_INVALID
    second = spans((0, 8), (8, 17))
    # a NULL output is refused before bad rows where the header lists it first ...
    refused(lib, c["hap"](windows=second, d_out=None), INVALID, "d_out is NULL")
    refused(lib, c["ehh"](r1=17, d_out=None), INVALID, "d_out is NULL")
    refused(lib, c["sfs"](windows=second, d_sfs=None), INVALID, "d_sfs is NULL")
    refused(lib, c["sfs_joint"](r0=1, d_sfs=None), INVALID, "d_sfs is NULL")
    refused(lib, c["fstat"](blocks=second, d_moments=None), INVALID, "d_moments is NULL")
    refused(lib, c["assoc"](r0=1, d_sum=None), INVALID, "d_dosage_sum is NULL")
    refused(lib, c["ld_band"](m=bytes_only, d_out=None), INVALID, "d_out is NULL")
    refused(lib, c["ld_prune"](r0=1, h_keep=None), INVALID, "h_keep is NULL")
    refused(lib, c["kinship"](r0=1, o=None), INVALID, "out is NULL")
    # ... and after them in fmh_genotype_counts; the sample list comes before the rows
    refused(lib, c["qc"](r0=1, s=None), INVALID, PAST)
    for name in ("qc", "assoc", "kinship"):
        refused(lib, c[name](samples=u32(0, 8), n=2, r0=1), INVALID, SAMPLE_RANGE)
    # bad rows are refused before the missing packed image
    refused(lib, c["hap"](m=bytes_only, windows=second), INVALID, "rows [8, 17) of window 1 exceed the matrix's 16 variants")
    refused(lib, c["ehh"](m=bytes_only, r1=17), INVALID, "rows [0, 17) exceed the matrix's 16 variants")
    refused(lib, c["sfs"](m=bytes_only, windows=second), INVALID, "rows [8, 17) of window 1 exceed the matrix's 16 variants")
    refused(lib, c["sfs_joint"](m=bytes_only, r0=1), INVALID, "rows [1, 17) of window 0 exceed the matrix's 16 variants")
    refused(lib, c["fstat"](m=bytes_only, blocks=second), INVALID, "rows [8, 17) of block 1 exceed the matrix's 16 variants")
    refused(lib, c["ld_band"](m=bytes_only, end=17), INVALID, "partner_end 17 exceeds the matrix's 16 variants")
    for name in ("qc", "assoc", "ld_prune", "kinship"):
        refused(lib, c[name](m=bytes_only, r0=1), INVALID, PAST)
    # no refusal left anything behind
    for name, call in c.items():
        assert call() == 0, (name, lib.fmh_last_error().decode())


# timing_add calls of one valid call
SPANS = dict(hap=1, ehh=1, sfs=1, sfs_joint=1, fstat=1, qc=1, hwe=1, assoc=1, ld_band=1, ld_prune=2, kinship=0)


def test_timing_accounting(frame):
    lib, _abi, c, _ = frame

    def read():
        ms, launches, gram = C.c_double(), C.c_uint64(), (C.c_double * 4)()
        assert lib.fmh_timing_read(C.byref(ms), C.byref(launches)) == 0 and lib.fmh_timing_read_gram(gram) == 0
        return ms.value, launches.value, list(gram)

    try:
        assert lib.fmh_timing_reset() == 0 and lib.fmh_timing_enable(1) == 0
        for name, call in c.items():
            ms0, launches0, _ = read()
            assert call() == 0, (name, lib.fmh_last_error().decode())
            ms1, launches1, gram = read()
            print(name, launches1 - launches0, ms1 - ms0, gram)
            assert launches1 - launches0 == SPANS[name], name
            if SPANS[name]:
                assert ms1 > ms0, name
            else:  # the Gram stage timer: per-stage times of the thread's last call, nothing added to the library's kernel time
                assert ms1 == ms0 and sum(gram) > 0.0, name
        assert lib.fmh_timing_enable(0) == 0
        before = read()
        for name, call in c.items():
            assert call() == 0, (name, lib.fmh_last_error().decode())
        assert read() == before
    finally:
        lib.fmh_timing_enable(0)
        lib.fmh_timing_reset()
