"""fmh_pairwise_differences against an all-pairs oracle at the size README and DESIGN 3.7 quote it at (1 M sites x 2 500 samples), at
every accepted ploidy, in both layouts and on every route the host picks from the shape.  Every output is an integer: every comparison
is array_equal over the WHOLE [n, n] matrices (upper triangle = the pairs, the rest must stay zero), no tolerance anywhere.

The oracle (oracle/dense_oracle.c fo_pairwise_differences_threaded, pinned to the Python restatement of stats.rs:4106-4231 by
tests/test_oracle_dense_c.py) works bit-parallel on haplotypes - XOR, AND, popcount - and shares no algebra with the kernels' per-allele
count planes and len * len - sum cnt * cnt.

Route table (pairwise.hip; CUS = 256 on an MI355X, G = CUS / 8 * 8 persistent workgroups; _route() below restates it and every case
prints and asserts the route it is there for):

  n_pad = round_up(n + [one-plane: 1 for the ones row], 256), nt = n_pad / 256, tiles = nt (nt + 1) / 2
  K bytes per sample kb = round_up(sites, ks) / spb; FP4 (ploidy <= 4): spb = 2, ks = 256; int8: spb = 1, ks = 128
  j = ceil(G / tiles) slices per XCD; k_chunk = round_up(ceil(kb / 8 j), 128), at least min(kb, 4096), at most
  k_cap = (2^24 [FP4] or 2^31 - 1 [int8]) / ploidy^2 sites; then j = ceil(ceil(kb / k_chunk) / 8)
  slab epilogue needs tiles x 8 x j x 256 KiB <= FMH_PD_SLAB_BYTES (4 GiB), else 64-bit atomics
  site slabs when n_planes x n_pad x sites / spb > FMH_PD_PLANES_BYTES (8 GiB); n_planes = 1, or alleles (+ 2 with missing calls)

  shape                                    nt  tiles  first j  k_chunk      j  epilogue            site slabs  why it is here
  600 x 70 000 (old suite's largest)        3      6       43     4 096     2  slabs               1           what was gated before
  2 500 x 1 M, one plane, FP4              10     55        5    12 544     5  slabs (0.58 GB)     1           the quoted size
  2 500 x 1 M, FMH_PD_INT8                 10     55        5    25 088     5  slabs               1           int8 at the quoted size
  2 500 x 1 M, alleles 0..5 + missing      10     55        5    10 496   5/3  slabs               2 (8 planes x 2 560 x 0.5 MB = 10.2 GB)
                                                                                                               default budget crossed; 3-plane unpack
  2 500 x 1 M, alleles 0..3 + missing      10     55        5    12 544     5  slabs               1 (6 planes = 7.7 GB)
  16 500 x 8 192                           65  2 145        1     4 096     1  atomics (4.50 GB)   1           default leaves the slabs
  16 500 x 8 192, FMH_PD_SLAB_BYTES 8 GiB  65  2 145        1     4 096     1  slabs               1           the same shape on slabs
  16 383 of 16 500                         64  2 080        1     4 096     1  atomics (4.36 GB)   1           first nt over the slab budget
  16 127 / 16 128 of 16 500             63/64  2 016/80     1     4 096     1  slabs / atomics     1           last nt inside; ones row opens tile 64
  ploidy 4, 10 M sites, FMH_PD_KCHUNK       1      1        -   <= k_cap    2  slabs               1           FP4 cap: 2^24 / 16 = 1 048 576 sites
  ploidy 127, 1.1 M sites, FMH_PD_KCHUNK    1      1        -   <= k_cap    2  slabs               1           int8 cap: (2^31 - 1) / 127^2 = 133 144
  ploidy 1..127 x 300, 2 500 sites          2      3       86     <= 4 096  1  slabs               1           planes kernels: prefix loops, LDS sizing

FMH_PD_OCC caps the workgroups per CU of the round-3 kernel (FMH_PD_PHASED=0) only, and that kernel's 128 KiB of LDS already leaves one
per CU on gfx950: with or without FMH_PD_PHASED=0 it is a NO-OP on this hardware.  Both spellings run because it is a documented switch;
neither counts as coverage of a different route.

The route assertions check _route(), a Python restatement of the host's arithmetic, not the route the library took: the library has no
query for that, so the two can drift apart unnoticed (for FMH_PD_PHASED=0 the restatement prints the phased grid's j; the host's grid there
is CUS x occupancy, the same number while the occupancy is 1).  The assertions keep the SHAPES honest - a case that stops reaching the
route it was written for fails - and the parity checks do not depend on them.

Every case prints its oracle wall time (16 threads).  The docstrings of test_ploidy_matrix, test_alleles_above_seven_are_u8_rows and
test_sample_subsets hold the times measured on an MI355X host; the full-size tests (headline, general, wide) only print theirs."""

import time

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H

pytestmark = pytest.mark.gpu

THREADS = 16  # the oracle's thread count: passed, never taken from the machine


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def cus():
    import ctypes as C

    from ferromic_amd import _abi

    n, mem = C.c_int(), C.c_uint64()
    _abi.check(_abi.load().fmh_device_info(0, C.create_string_buffer(128), 128, C.byref(n), C.byref(mem)))
    return n.value


def _round_up(a, b):
    return (a + b - 1) // b * b


def _route(cus, n, sites, ploidy, max_allele, missing, int8=False, two_planes=False, kchunk=0, slabs=True, slab_bytes=4 << 30,
           planes_bytes=8 << 30, phased=True):
    """pairwise.hip's host decisions for one call, restated (see the table in the module docstring)."""
    n_alleles = max_allele + 1
    single = not missing and n_alleles == 2 and not two_planes
    n_planes = 1 if single else (n_alleles + 2 if missing else n_alleles)
    n_pad = _round_up(n + (1 if single else 0), 256)
    fp4 = ploidy <= 4 and not int8
    spb = 2 if fp4 else 1
    ksites = 128 * spb
    slab = max(planes_bytes // (n_planes * n_pad), 128) // 128 * ksites
    slab = min(_round_up(sites, ksites), slab)
    nt = n_pad // 256
    tiles = nt * (nt + 1) // 2
    grid = max(8, cus // 8 * 8)
    out = []
    for row0 in range(0, sites, slab):
        rows = min(slab, sites - row0)
        kb = _round_up(rows, ksites) // spb
        j = max(1, -(-kb // (8 * kchunk))) if kchunk else max(1, -(-grid // tiles))
        cap_sites = ((1 << 24) if fp4 else ((1 << 31) - 1)) // (ploidy * ploidy)
        k_cap = max(cap_sites // spb // 128, 1) * 128
        k_chunk = _round_up(-(-kb // (8 * j)), 128)
        k_chunk = max(k_chunk, min(kb, 4096))
        capped = k_chunk > k_cap
        k_chunk = min(k_chunk, k_cap)
        j = (-(-kb // k_chunk) + 7) // 8
        need = tiles * 8 * j * 256 * 256 * 4
        out.append(dict(rows=rows, j=j, k_chunk=k_chunk, capped=capped, epilogue="slabs" if phased and slabs and need <= slab_bytes else "atomics", slab_need=need))
    return dict(single=single, fp4=fp4, n_planes=n_planes, nt=nt, tiles=tiles, site_slabs=len(out), per_slab=out)


def _route_text(r):
    s = r["per_slab"][0]
    return (f"{'one plane' if r['single'] else str(r['n_planes']) + ' planes'}, {'FP4' if r['fp4'] else 'int8'}, nt {r['nt']}, tiles {r['tiles']}, "
            f"j {s['j']}, k_chunk {s['k_chunk']}{' (capped)' if s['capped'] else ''}, {s['epilogue']} ({s['slab_need'] / 1e9:.2f} GB), site slabs {r['site_slabs']}")


def _oracle(data, words, sites, stride, ploidy, n, max_allele):
    t0 = time.perf_counter()
    diff, both = D.pairwise_differences(data, words, sites, stride, ploidy, n, max_allele, THREADS)
    return diff, both, time.perf_counter() - t0


def _same(got, exp, what):
    """Whole-matrix equality; on a mismatch say how many entries differ and where the first one sits in the 256-tiling."""
    assert got.shape == exp.shape, what
    if np.array_equal(got, exp):
        return
    bad = np.argwhere(got != exp)
    i, j = (int(x) for x in bad[0])
    tiles = sorted({(int(a) // 256, int(b) // 256) for a, b in bad[:: max(1, len(bad) // 4096)]})
    raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ; first ({i}, {j}) tile ({i // 256}, {j // 256}): gpu={int(got[i, j])} "
                         f"oracle={int(exp[i, j])}; tiles hit (sampled): {tiles[:24]}")


def _check(dev, dm, n, exp_diff, exp_both, what):
    diff, both = dev.pairwise_differences(dm, n)
    _same(diff, exp_diff, f"diff, {what}")
    _same(both, exp_both, f"both, {what}")


def _missing_words(miss):
    bits = np.packbits(miss.reshape(-1), bitorder="little")
    return np.frombuffer(np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).tobytes(), dtype="<u8").copy()


def _random_cohort(rng, sites, samples, ploidy, max_allele, p_missing):
    """Mostly biallelic, mostly complete rows with a minority (a fifth) of general rows, like real data; the first row is general and
    meets the declared max_allele."""
    Hc = samples * ploidy
    data = (rng.random((sites, Hc), dtype=np.float32) < rng.beta(0.8, 0.8, size=(sites, 1)).astype(np.float32)).astype(np.uint8)
    general = rng.random(sites) < 0.2
    general[0] = True
    g = np.nonzero(general)[0]
    if max_allele > 1:
        sub = rng.integers(0, max_allele + 1, size=(len(g), Hc), dtype=np.uint8)
        sub[rng.random((len(g), Hc), dtype=np.float32) < 0.4] = 0
        data[g] = sub
        data[0, 0] = max_allele
    words = None
    if p_missing > 0:
        miss = np.zeros((sites, Hc), dtype=bool)
        miss[g] = rng.random((len(g), Hc), dtype=np.float32) < p_missing * 5  # all of the missing calls sit in the general rows
        miss[0, 0] = False
        miss[0, Hc - 1] = True  # the last slot of the last sample, whatever the draw
        data[miss] = 0
        words = _missing_words(miss)
    return data, words


def _from_host(dev, fmh_opts, layout, data, words, sites, samples, ploidy, max_allele):
    """`packed`: what fmh_matrix_create keeps by default (bit planes only, alleles 0..7); `bytes`: the u8 rows (FMH_LAYOUT=bytes at create
    time keeps them, and keeps the u8 kernels on them)."""
    if layout == "bytes":
        fmh_opts.setenv("FMH_LAYOUT", "bytes")
    else:
        fmh_opts.delenv("FMH_LAYOUT")
    return dev.DeviceMatrix.from_host(data.reshape(-1), words, sites, samples, ploidy, max_allele)


# ---- headline: the quoted size ---------------------------------------------------------------------------------------------------------


def test_headline_1m_sites_2500_samples(dev, fmh_opts, cus):
    """1 M sites x 2 500 diploid samples, biallelic, complete, generated on the device and regenerated on the host from the same stream:
    all 3 123 750 pairs, u8 rows and bit planes, and on the packed matrix every Gram route (int8, two planes, round-3 kernel, atomic
    epilogue) against ONE oracle run; both == sites for every pair."""
    S, N = 1_000_000, 2500
    seed = S + N
    thr = H.thresholds(S, seed)
    poc = np.repeat((np.arange(N) >= N // 2).astype(np.uint8), 2)
    dm = dev.DeviceMatrix.alloc(S, N, 2, with_missing=False)
    dm.generate(seed, 0, thr, poc, 0)
    hdata, _ = D.generate(S, 2 * N, seed, 0, thr, poc, 0, THREADS)
    assert np.array_equal(dm.download()[0], hdata)  # the host generator is the same stream
    exp_diff, exp_both, secs = _oracle(hdata, None, S, 2 * N, 2, N, 1)
    del hdata
    r = _route(cus, N, S, 2, 1, False)
    print(f"\nheadline {S} x {N}: {_route_text(r)}; oracle {secs:.1f} s on {THREADS} threads")
    assert r["single"] and r["fp4"] and r["site_slabs"] == 1 and r["per_slab"][0]["epilogue"] == "slabs" and 1 < r["per_slab"][0]["j"] < 43
    iu = np.triu_indices(N, k=1)
    assert (exp_both[iu] == S).all() and not np.tril(exp_both).any()
    _check(dev, dm, N, exp_diff, exp_both, "bytes (u8 rows only)")
    fmh_opts.setenv("FMH_PD_SB", "32")
    _check(dev, dm, N, exp_diff, exp_both, "bytes, FMH_PD_SB=32")
    fmh_opts.delenv("FMH_PD_SB")
    dm.pack(release_bytes=False)
    fmh_opts.setenv("FMH_LAYOUT", "bytes")
    _check(dev, dm, N, exp_diff, exp_both, "bytes (FMH_LAYOUT=bytes beside a packed image)")
    fmh_opts.delenv("FMH_LAYOUT")
    dm.pack(release_bytes=True)
    _check(dev, dm, N, exp_diff, exp_both, "packed")
    for key, value in (("FMH_PD_INT8", "1"), ("FMH_PD_TWO_PLANES", "1"), ("FMH_PD_PHASED", "0"), ("FMH_PD_SLABS", "0"), ("FMH_PD_OCC", "1"), ("FMH_PD_SB", "32")):
        fmh_opts.setenv(key, value)
        kw = dict(int8=key == "FMH_PD_INT8", two_planes=key == "FMH_PD_TWO_PLANES", phased=key != "FMH_PD_PHASED", slabs=key != "FMH_PD_SLABS")
        print(f"  packed, {key}={value}: {_route_text(_route(cus, N, S, 2, 1, False, **kw))}")
        _check(dev, dm, N, exp_diff, exp_both, f"packed, {key}={value}")
        fmh_opts.delenv(key)
    # FMH_PD_OCC on the one kernel whose grid it enters (round 3's), set in the running process
    fmh_opts.setenv("FMH_PD_PHASED", "0")
    fmh_opts.setenv("FMH_PD_OCC", "1")
    _check(dev, dm, N, exp_diff, exp_both, "packed, FMH_PD_PHASED=0 FMH_PD_OCC=1")


# ---- general data at scale ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("max_allele,site_slabs", [(5, 2), (3, 1)])
def test_general_1m_sites_2500_samples(dev, fmh_opts, cus, max_allele, site_slabs):
    """1 M sites x 2 500 diploid samples, mostly biallelic complete rows, 2 % multi-allelic rows and 1 % rows with missing calls
    (helpers.build_cohort: the cohort of the full-size sweep gates), all pairs, both layouts.
    max_allele 5: 6 allele planes + length + valid = 8 FP4 planes x 2 560 padded samples x 500 000 B = 10.24 GB > the 8 GiB planes budget, so
      the site axis is cut in two slabs (838 656 + 161 344 sites) BY DEFAULT; the packed image has three bit planes and is unpacked slab by slab.
    max_allele 3: 6 planes = 7.68 GB, one slab; the packed image has two bit planes and feeds the packed planes kernel directly."""
    S, N = 1_000_000, 2500
    data, words, _ = H.build_cohort(S, N, 4106 + max_allele, 0.02, max_allele, 0.01, N // 2)
    exp_diff, exp_both, secs = _oracle(data, words, S, 2 * N, 2, N, max_allele)
    r = _route(cus, N, S, 2, max_allele, True)
    print(f"\ngeneral {S} x {N}, alleles 0..{max_allele}, missing calls: {_route_text(r)}; oracle {secs:.1f} s on {THREADS} threads")
    assert not r["single"] and r["fp4"] and r["n_planes"] == max_allele + 3 and r["site_slabs"] == site_slabs
    iu = np.triu_indices(N, k=1)
    assert exp_both[iu].min() < S and exp_both[iu].max() <= S  # the missing calls reach the pairs
    for layout in ("packed", "bytes"):
        dm = _from_host(dev, fmh_opts, layout, data, words, S, N, 2, max_allele)
        _check(dev, dm, N, exp_diff, exp_both, layout)
        dm.close()


# ---- wide: more tile pairs than workgroups, the slab budget --------------------------------------------------------------------------------


def test_wide_16500_samples(dev, fmh_opts, cus):
    """16 500 samples x 8 192 sites, biallelic, complete, all 136 M pairs: nt = 65, 2 145 tile pairs > 256 workgroups so j = 1, and the
    slab epilogue would need 2 145 x 8 x 256 KiB = 4.50 GB > FMH_PD_SLAB_BYTES = 4 GiB: the DEFAULT is the 64-bit atomic epilogue.  The same
    shape with the budget raised to 8 GiB takes the slabs; both must equal the oracle.  Then the first n samples of the same matrix (the
    ones row of the one-plane route then sits in the middle of the matrix) around the budget boundary nt = 63 -> 64, all pairs each
    (a superset of sampled pairs + the last tile row), against the oracle's [:n, :n] block (tests/test_oracle_dense_c.py pins that a
    subset's result is that block): 16 127 (nt 63, slabs by default), 16 128 (the ones row opens tile 64: atomics), 16 383 (nt 64, the
    ones row is the last row of the last tile: atomics)."""
    S, N = 8192, 16_500
    seed = S + N
    thr = H.thresholds(S, seed)
    poc = np.repeat((np.arange(N) >= N // 2).astype(np.uint8), 2)
    hdata, _ = D.generate(S, 2 * N, seed, 0, thr, poc, 0, THREADS)
    exp_diff, exp_both, secs = _oracle(hdata, None, S, 2 * N, 2, N, 1)
    r = _route(cus, N, S, 2, 1, False)
    print(f"\nwide {S} x {N}: {_route_text(r)}; oracle {secs:.1f} s on {THREADS} threads")
    assert r["nt"] == 65 and r["per_slab"][0]["j"] == 1 and r["per_slab"][0]["epilogue"] == "atomics"
    dm = dev.DeviceMatrix.from_host(hdata, None, S, N, 2, 1)
    del hdata
    _check(dev, dm, N, exp_diff, exp_both, "default (atomics)")
    fmh_opts.setenv("FMH_PD_SLAB_BYTES", str(8 << 30))
    r = _route(cus, N, S, 2, 1, False, slab_bytes=8 << 30)
    print(f"  FMH_PD_SLAB_BYTES=8 GiB: {_route_text(r)}")
    assert r["per_slab"][0]["epilogue"] == "slabs"
    _check(dev, dm, N, exp_diff, exp_both, "FMH_PD_SLAB_BYTES raised (slabs)")
    fmh_opts.delenv("FMH_PD_SLAB_BYTES")
    for n, nt, epilogue in ((16_127, 63, "slabs"), (16_128, 64, "atomics"), (16_383, 64, "atomics")):
        r = _route(cus, n, S, 2, 1, False)
        print(f"  first {n} samples: {_route_text(r)}")
        assert r["nt"] == nt and r["per_slab"][0]["epilogue"] == epilogue
        _check(dev, dm, n, np.ascontiguousarray(exp_diff[:n, :n]), np.ascontiguousarray(exp_both[:n, :n]), f"first {n} samples")


# ---- every accepted ploidy -------------------------------------------------------------------------------------------------------------

PLOIDIES = [1, 3, 4, 5, 8, 13, 14, 32, 127]


@pytest.mark.parametrize("ploidy", PLOIDIES)
def test_ploidy_matrix(dev, fmh_opts, cus, ploidy):
    """300 samples (two 256-sample tiles) x 2 500 sites at ploidy 1, 3, 4 (FP4) and 5 .. 127 (int8 by ploidy), complete and with missing
    calls, biallelic and alleles 0..3, bit planes and u8 rows: all pairs.  With missing calls or alleles above 1 a ploidy other than 2
    runs the per-allele prefix loop of both planes kernels.
    Ploidy >= 14 on the packed layout: the packed planes kernel staged 256 samples per workgroup = 3 x 128 x (256 x ploidy / 8 + 1) B of
    LDS, 172 416 B > 160 KiB at ploidy 14; observed once with the earlier code on an MI355X: FMH_ERR_HIP ("invalid argument"), an error
    return and no launch, as the arithmetic predicts.  pairwise.hip now halves the samples per
    workgroup until the tile fits, and these cases assert parity.
    Oracle, 16 threads of the MI355X host, per cohort: 0.0 s up to ploidy 14, 0.1-0.2 s at ploidy 32, 1.7-1.8 s (biallelic) and 3.6-3.8 s
    (alleles 0..3) at ploidy 127."""
    S, N = 2500, 300
    rng = np.random.default_rng(1000 + ploidy)
    for max_allele in (1, 3):
        for p_missing in (0.0, 0.03):
            data, words = _random_cohort(rng, S, N, ploidy, max_allele, p_missing)
            exp_diff, exp_both, secs = _oracle(data, words, S, N * ploidy, ploidy, N, max_allele)
            r = _route(cus, N, S, ploidy, max_allele, words is not None)
            print(f"\nploidy {ploidy}, alleles 0..{max_allele}, missing {p_missing}: {_route_text(r)}; oracle {secs:.1f} s on {THREADS} threads")
            assert r["fp4"] == (ploidy <= 4) and r["nt"] == 2
            for layout in ("packed", "bytes"):
                dm = _from_host(dev, fmh_opts, layout, data, words, S, N, ploidy, max_allele)
                _check(dev, dm, N, exp_diff, exp_both, f"ploidy {ploidy}, alleles 0..{max_allele}, missing {p_missing}, {layout}")
                dm.close()


@pytest.mark.parametrize("ploidy", [2, 3])
@pytest.mark.parametrize("max_allele", [9, 15])
def test_alleles_above_seven_are_u8_rows(dev, cus, ploidy, max_allele):
    """max_allele 9 and 15: beyond the packed layout (alleles 0..7), so u8 rows by necessity; 10 / 16 allele planes, + 2 with missing calls.
    Oracle, 16 threads of the MI355X host: under 0.05 s per cohort."""
    S, N = 3000, 300
    rng = np.random.default_rng(max_allele * 10 + ploidy)
    for p_missing in (0.0, 0.03):
        data, words = _random_cohort(rng, S, N, ploidy, max_allele, p_missing)
        exp_diff, exp_both, secs = _oracle(data, words, S, N * ploidy, ploidy, N, max_allele)
        r = _route(cus, N, S, ploidy, max_allele, words is not None)
        print(f"\nploidy {ploidy}, alleles 0..{max_allele}, missing {p_missing}: {_route_text(r)}; oracle {secs:.1f} s on {THREADS} threads")
        assert r["n_planes"] == max_allele + 1 + (2 if words is not None else 0)
        dm = dev.DeviceMatrix.from_host(data.reshape(-1), words, S, N, ploidy, max_allele)
        _check(dev, dm, N, exp_diff, exp_both, f"ploidy {ploidy}, alleles 0..{max_allele}, missing {p_missing}")
        dm.close()


@pytest.mark.parametrize("layout", ["packed", "bytes"])
@pytest.mark.parametrize("max_allele,p_missing", [(1, 0.0), (3, 0.03)])
def test_sample_subsets(dev, fmh_opts, cus, layout, max_allele, p_missing):
    """n_samples < samples on a 600-sample diploid matrix: 1 (nothing to do), 2, 255, 256, 257, 512 and samples - 1, against the oracle
    restricted to those samples.  On the one-plane route the ones row then overwrites sample n_samples' place in the middle of the
    matrix; at 256 and 512 it opens a tile of its own.
    Oracle, 16 threads of the MI355X host: 0.01 s or less per subset."""
    S, N = 5000, 600
    data, words = _random_cohort(np.random.default_rng(600 + max_allele), S, N, 2, max_allele, p_missing)
    dm = _from_host(dev, fmh_opts, layout, data, words, S, N, 2, max_allele)
    for n in (1, 2, 255, 256, 257, 512, N - 1, N):
        exp_diff, exp_both, secs = _oracle(data, words, S, N * 2, 2, n, max_allele)
        print(f"\nfirst {n} of {N} samples, alleles 0..{max_allele}, missing {p_missing}, {layout}: {_route_text(_route(cus, n, S, 2, max_allele, words is not None))}; "
              f"oracle {secs:.2f} s on {THREADS} threads")
        _check(dev, dm, n, exp_diff, exp_both, f"first {n} samples, {layout}")


# ---- the exactness caps ------------------------------------------------------------------------------------------------------------------


def _mismatch_counts(g):
    """diff of every pair by comparing haplotype columns directly (complete data): sum over sites and allele pairs of [a != b]."""
    S, N, ploidy = g.shape
    h = np.ascontiguousarray(g.reshape(S, N * ploidy).T)  # haplotype-major
    out = np.zeros((N, N), dtype=np.uint64)
    for i in range(N):
        for j in range(i + 1, N):
            out[i, j] = sum(int(np.count_nonzero(h[i * ploidy + a] != h[j * ploidy + b])) for a in range(ploidy) for b in range(ploidy))
    return out


def test_fp4_cap_ploidy_4(dev, fmh_opts, cus):
    """Ploidy 4 is the largest FP4 code: products up to 16, f32 accumulators exact up to 2^24, so an item may span 2^24 / 16 = 1 048 576
    sites.  10 M sites with FMH_PD_KCHUNK huge ask for ONE slice per XCD = 1.25 M sites per item: the host must cap it.  Samples 0 and 1
    are all-ones genotypes (an uncapped item sums 16 x 1.25 M = 2 x 10^7 > 2^24); all-ones alone cannot show a lost cap - multiples of
    16 stay exact in f32 up to 2^28.  What can show it are ODD sums per MFMA instruction (one v_mfma_scale_f32_16x16x128_f8f6f4 spans 128
    consecutive sites): samples 2 and 3 carry a single 1 at every 128th site, so pair (2, 3) adds 127 x 16 + 1 per instruction, and sample 5
    holds a 3 at every third site, so its pairs with 0..3 add odd or even sums in turn; beyond 2^24 an f32 accumulator cannot hold an odd
    sum.  Observed once on an MI355X with the cap taken out by hand (the int8 bound in place of 2^24): this test fails, 3 of the 15 pairs
    differ, the first of them pair (2, 3) with 492 968 where 468 750 is right; the old test_pairwise_* stay green under that mutation.
    Expected values by comparing haplotype columns in numpy."""
    S, N, ploidy = 10_000_000, 6, 4
    g = np.ones((S, N, ploidy), dtype=np.uint8)
    g[::128, 2, 1:] = 0
    g[::128, 3, 1:] = 0
    g[:, 4, :] = 0
    g[::3, 5, 0] = 0
    exp_diff = _mismatch_counts(g)
    assert exp_diff[0, 1] == 0 and exp_diff[0, 4] == 16 * S and exp_diff[2, 3] == 6 * ((S + 127) // 128)
    exp_both = np.triu(np.full((N, N), S, dtype=np.uint64), 1)
    dm = dev.DeviceMatrix.from_host(g.reshape(-1), None, S, N, ploidy, 1)
    for kchunk in (100_000_000, 0):
        for two_planes in (False, True):
            r = _route(cus, N, S, ploidy, 1, False, two_planes=two_planes, kchunk=kchunk)
            print(f"\nFP4 cap, FMH_PD_KCHUNK={kchunk}, two planes {two_planes}: {_route_text(r)}")
            assert r["fp4"] and r["per_slab"][0]["capped"] == (kchunk > 0)
            fmh_opts.setenv("FMH_PD_KCHUNK", str(kchunk))
            fmh_opts.setenv("FMH_PD_TWO_PLANES", "1" if two_planes else "0")
            _check(dev, dm, N, exp_diff, exp_both, f"FMH_PD_KCHUNK={kchunk}, two planes {two_planes}")


def test_int8_cap_ploidy_127(dev, fmh_opts, cus):
    """Ploidy 127 is the largest int8 operand: products up to 16 129, int32 accumulators, so an item may span (2^31 - 1) / 127^2 =
    133 144 sites.  1.1 M sites with FMH_PD_KCHUNK huge ask for 137 500 sites per item: uncapped, the all-ones pair sums 2.2 x 10^9 >
    2^31.  Every genotype is constant over the sites, so the expected values are closed-form: diff(i, j) = sites x (ones_i zeros_j +
    zeros_i ones_j)."""
    S, N, ploidy = 1_100_000, 4, 127
    ones = [127, 127, 0, 60]
    row = np.zeros((N, ploidy), dtype=np.uint8)
    for i, c in enumerate(ones):
        row[i, :c] = 1
    exp_diff = np.zeros((N, N), dtype=np.uint64)
    for i in range(N):
        for j in range(i + 1, N):
            exp_diff[i, j] = S * (ones[i] * (ploidy - ones[j]) + (ploidy - ones[i]) * ones[j])
    exp_both = np.triu(np.full((N, N), S, dtype=np.uint64), 1)
    data = np.broadcast_to(row.reshape(1, -1), (S, N * ploidy))
    for layout in ("packed", "bytes"):
        dm = _from_host(dev, fmh_opts, layout, np.ascontiguousarray(data), None, S, N, ploidy, 1)
        for kchunk in (100_000_000, 0):
            for two_planes in (False, True):
                r = _route(cus, N, S, ploidy, 1, False, two_planes=two_planes, kchunk=kchunk)
                print(f"\nint8 cap, {layout}, FMH_PD_KCHUNK={kchunk}, two planes {two_planes}: {_route_text(r)}")
                assert not r["fp4"] and r["per_slab"][0]["capped"] == (kchunk > 0)
                fmh_opts.setenv("FMH_PD_KCHUNK", str(kchunk))
                fmh_opts.setenv("FMH_PD_TWO_PLANES", "1" if two_planes else "0")
                _check(dev, dm, N, exp_diff, exp_both, f"{layout}, FMH_PD_KCHUNK={kchunk}, two planes {two_planes}")
        dm.close()
