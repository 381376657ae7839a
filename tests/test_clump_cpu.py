"""LD clumping where no device is needed: the oracle (tests/clump_ref.py) against numpy, the host-only entry points fmh_geno_ld_r2,
fmh_geno_ld_pairs_host and fmh_clump_host against the oracle (integers and assignments with array_equal, r^2 bit for bit), the exact 1.0
of duplicated and complemented rows, the NaN of monomorphic ones, the refusals of the host entry points and of NULL pointers in the
header's order, the Python argument errors and the empty answers of ferromic.ld_clump / genotype_ld, and the twin run stand-alone under
ASan and UBSan (ferromic_amd/csrc/clump_host_check.cpp), whose checksum line is compared with the oracle's over a splitmix64 cohort that
tests/clump_ref.py restates."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import clump_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.path.join(ROOT, "ferromic_amd", "bin")


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm(dev):
    import ferromic

    return ferromic


def index_array(got, dev):
    return np.where(got.index_of == dev.CLUMP_NONE, -1, got.index_of.astype(np.int64))


def check_twin(dev, d, x, p, prm, what):
    ref = R.clump(d, x, p, prm)
    got = dev.clump_host(d, p, dev.clump_params(**prm), x=x)
    assert np.array_equal(index_array(got, dev), ref["index_of"]), what
    assert R.same_bits(got.r2, ref["r2"]), what
    assert got.n_clumps == ref["n_clumps"], what
    assert np.array_equal(index_array(dev.clump_host(d, p, dev.clump_params(**prm), x=x, want_r2=False), dev), ref["index_of"]), what
    return ref


def test_oracle_r2_is_pearson():
    d = R.mosaic_dosages(60, 41, 7)
    checked = 0
    for a in range(0, 60, 3):
        for b in range(a, 60, 7):
            both = (d[a] < 3) & (d[b] < 3)
            v = R.r2_of(R.counts(d[a], d[b]))
            ga, gb = d[a][both].astype(float), d[b][both].astype(float)
            if ga.std() == 0 or gb.std() == 0:
                assert math.isnan(v)
                continue
            assert abs(v - np.corrcoef(ga, gb)[0, 1] ** 2) <= 1e-9, (a, b)
            checked += 1
    assert checked > 50


def test_counts_and_r2_against_the_oracle(dev):
    d = R.mosaic_dosages(80, 37, 3)
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 80, size=300), rng.integers(0, 80, size=300)
    a[:5], b[:5] = [0, 0, 0, 79, 78], [0, 1, 2, 79, 5]                              # a == b, the duplicate, the complement, monomorphic rows
    want = R.pair_counts(d, a, b)
    got = dev.geno_ld_pairs_host(d, a, b)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    r2 = dev.geno_ld_r2(got)
    assert R.same_bits(r2, [R.r2_of(c) for c in want])
    assert r2[0] == 1.0 and r2[1] == 1.0 and r2[2] == 1.0 and math.isnan(r2[3]) and math.isnan(r2[4])
    assert dev.geno_ld_pairs_host(d, [], []).shape == (0, 6) and dev.geno_ld_r2(np.zeros((0, 6))).shape == (0,)
    # the formula alone, on integers near its limits: 600 000 columns of dosage 2 keep every product below 2^53
    big = np.array([[300_000, 300_001, 299_999, 600_004, 599_990, 300_003], [0, 0, 0, 0, 0, 0], [5, 5, 5, 5, 9, 7]], dtype=np.int64)
    assert R.same_bits(dev.geno_ld_r2(big), [R.r2_of(c) for c in big]) and math.isnan(dev.geno_ld_r2(big)[1])


@pytest.mark.parametrize("seed", [1, 2])
def test_twin_against_the_oracle(dev, seed):
    d, x, p = R.mosaic_dosages(300, 37, seed), R.mosaic_positions(300, seed), R.mosaic_p(300, seed)
    ref = check_twin(dev, d, x, p, R.params(p1=0.03, p2=0.1, r2=0.3, window=90), ("mosaic", seed))
    assert sum(1 for s in R.sizes(ref) if s >= 2) >= 20 and ref["unassigned"] >= 1 and ref["claimed_before_turn"] >= 1
    check_twin(dev, d, None, p, R.params(p1=0.05, p2=0.12, r2=0.0, window=7), ("rows as positions, r2 0", seed))
    check_twin(dev, d, x, p, R.params(p1=0.12, p2=0.12, r2=1.0, window=2**32 - 1), ("every site a candidate, r2 1", seed))
    check_twin(dev, d, x, p, R.params(p1=0.0, p2=0.0, r2=0.5, window=0), ("only p = 0, window 0", seed))
    none = check_twin(dev, d, x, np.full(300, np.nan), R.params(), "every p NaN")
    assert none["n_clumps"] == 0 and (none["index_of"] == -1).all()
    assert check_twin(dev, d[:0], x[:0], p[:0], R.params(), "no row")["n_clumps"] == 0


def test_duplicates_complements_and_monomorphic_rows(dev):
    d = R.mosaic_dosages(40, 25, 5, miss=0.1)
    p = np.full(40, 0.5)
    p[0] = 0.0                                                                       # row 0 is the first index
    p[39] = 1e-9                                                                     # a monomorphic candidate: an index that claims nothing
    ref = check_twin(dev, d, None, p, R.params(p1=0.01, p2=1.0, r2=1.0, window=100), "r2 = 1")
    assert ref["index_of"][:3].tolist() == [0, 0, 0] and ref["r2"][:3].tolist() == [1.0, 1.0, 1.0]
    assert ref["index_of"][39] == 39 and math.isnan(ref["r2"][39]) and (ref["index_of"] == 39).sum() == 1
    assert ref["index_of"][38] == -1 and math.isnan(ref["r2"][38])                   # NaN never qualifies, even at r2 = 0
    zero = check_twin(dev, d, None, p, R.params(p1=0.01, p2=1.0, r2=0.0, window=100), "r2 = 0")
    defined = [j for j in range(39) if not math.isnan(R.r2_of(R.counts(d[0], d[j])))]   # r2 = 0 claims every defined pair of the window
    assert zero["index_of"][38] == -1 and np.flatnonzero(zero["index_of"] == 0).tolist() == defined and len(defined) >= 30


def test_host_refusals_in_order(dev):
    lib, abi = dev._abi.load(), dev._abi
    d = np.zeros((3, 2), dtype=np.uint8)
    p = np.array([0.1, 0.2, 0.3])
    x = np.array([5, 4, 6], dtype=np.uint32)
    index_of = np.zeros(3, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    prm = dev.clump_params()

    def status(call):
        s = call()
        return s, lib.fmh_last_error().decode()

    host = lib.fmh_clump_host
    bad = dev.clump_params(p1=0.5, p2=0.1)
    assert status(lambda: host(ptr(d), None, ptr(p), 3, 2, None, ptr(index_of), None, None)) == (abi.FMH_ERR_INVALID, "NULL params")
    assert status(lambda: host(ptr(d), None, None, 3, 2, C.byref(bad), None, None, None)) == (abi.FMH_ERR_INVALID, "NULL h_p")
    assert status(lambda: host(ptr(d), None, ptr(p), 3, 0, C.byref(bad), None, None, None)) == (abi.FMH_ERR_INVALID, "NULL h_index_of")
    assert status(lambda: host(None, None, ptr(p), 3, 0, C.byref(bad), ptr(index_of), None, None)) == (abi.FMH_ERR_INVALID, "n_samples is 0")
    assert status(lambda: host(None, None, ptr(p), 3, 2, C.byref(bad), ptr(index_of), None, None)) == (abi.FMH_ERR_INVALID, "NULL dosage")
    four = np.array([[0, 1], [4, 1], [0, 0]], dtype=np.uint8)
    assert status(lambda: host(ptr(four), ptr(x), ptr(p), 3, 2, C.byref(bad), ptr(index_of), None, None))[1] == "dosage 4 (row 1, sample 0) is not 0, 1, 2 or 3"
    s, message = status(lambda: host(ptr(d), ptr(x), ptr(np.array([0.1, 2.0, 0.3])), 3, 2, C.byref(bad), ptr(index_of), None, None))
    assert s == abi.FMH_ERR_INVALID and message.startswith("0 <= p1 <= p2 <= 1 is required")
    for kw in (dict(p1=math.nan), dict(r2=math.nan)):
        assert status(lambda: host(ptr(d), ptr(x), ptr(p), 3, 2, C.byref(dev.clump_params(**kw)), ptr(index_of), None, None))[1].startswith("a parameter is NaN")
    assert status(lambda: host(ptr(d), ptr(x), ptr(p), 3, 2, C.byref(dev.clump_params(r2=1.5)), ptr(index_of), None, None))[1].startswith("0 <= r2 <= 1 is required")
    s, message = status(lambda: host(ptr(d), ptr(x), ptr(np.array([0.1, 2.0, 0.3])), 3, 2, C.byref(prm), ptr(index_of), None, None))
    assert (s, message) == (abi.FMH_ERR_INVALID, "p 2 of row 1 is neither NaN nor within [0, 1]")
    assert status(lambda: host(ptr(d), ptr(x), ptr(p), 3, 2, C.byref(prm), ptr(index_of), None, None)) == (abi.FMH_ERR_INVALID, "the positions descend at row 1")
    # the device calls: what is refused before a matrix is looked at
    assert status(lambda: lib.fmh_clump(None, None, 2, 0, 3, None, None, ptr(p), C.byref(prm), ptr(index_of), None, None, None)) == (abi.FMH_ERR_INVALID, "NULL matrix")
    assert status(lambda: lib.fmh_geno_ld_pairs(None, None, 2, None, None, 0, None, None)) == (abi.FMH_ERR_INVALID, "NULL matrix")
    # the pairs twin and the formula
    pairs = lib.fmh_geno_ld_pairs_host
    rows = np.array([0, 3], dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    assert status(lambda: pairs(ptr(d), 3, 0, ptr(rows), ptr(rows), 2, ptr(out))) == (abi.FMH_ERR_INVALID, "n_samples is 0")
    assert status(lambda: pairs(ptr(d), 3, 2, None, ptr(rows), 2, ptr(out))) == (abi.FMH_ERR_INVALID, "a NULL row list or output with 2 pairs")
    assert status(lambda: pairs(ptr(d), 3, 2, ptr(rows), ptr(rows), 2, ptr(out))) == (abi.FMH_ERR_INVALID, "pair 1 names rows (3, 3) of 3 rows")
    assert status(lambda: lib.fmh_geno_ld_r2(None, 2, None)) == (abi.FMH_ERR_INVALID, "NULL counts or output with 2 records")
    assert lib.fmh_geno_ld_r2(None, 0, None) == abi.FMH_OK and pairs(ptr(d), 3, 2, None, None, 0, None) == abi.FMH_OK


def records(n_sites=5, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, (i * s) & 1] for s in range(n_samples)]) for i in range(n_sites)]


def refused(message, call, kind=ValueError):
    with pytest.raises(kind) as caught:
        call()
    assert str(caught.value) == message, (str(caught.value), message)


def empty(c, rows):
    assert len(c) == 0 and repr(c) == "Clumps(clumps=0, rows=%d, assigned=0)" % rows
    for name, dtype in (("index_rows", np.int64), ("index_p", np.float64), ("sizes", np.int64)):
        assert getattr(c, name).dtype == dtype and getattr(c, name).shape == (0,), name
    assert c.clump_of.dtype == np.int64 and c.clump_of.tolist() == [-1] * rows and c.index_of.tolist() == [-1] * rows
    assert c.r2.dtype == np.float64 and c.r2.shape == (rows,) and np.isnan(c.r2).all()
    assert c.index_mask().dtype == np.bool_ and c.index_mask().tolist() == [False] * rows
    refused("clump 0 of 0", lambda: c.members(0), IndexError)


def test_python_surface_without_a_device(fm):
    V = records()
    assert fm.Clumps.__module__.endswith("_core") and callable(fm.ld_clump) and callable(fm.genotype_ld) and hasattr(fm.Population, "ld_clump")
    p = np.array([0.5, 0.2, np.nan, 0.9, 0.3])
    c = fm.ld_clump(V, p)                                                           # no p <= p2 = 0.01: no participant
    empty(c, 5)
    assert c.positions.tolist() == [0, 10, 20, 30, 40] and c.params == dict(p1=1e-4, p2=1e-2, r2=0.5, window=250_000)
    empty(fm.ld_clump(V, p, p1=0.1, p2=0.95), 5)                                    # participants, but no candidate
    empty(fm.ld_clump(V, np.zeros(5), sites=np.zeros(5, dtype=bool)), 5)            # no kept row
    empty(fm.ld_clump(V, np.zeros(0), region=(1000, 2000)), 0)
    pop = fm.Population.from_numpy("p", np.zeros((4, 3, 2), dtype=np.int8), np.arange(4) * 10, [(0, 0), (0, 1), (2, 0)], 100)
    empty(pop.ld_clump(np.full(4, 0.5)), 4)
    # argument errors, the parameters first
    refused("0 <= p1 <= p2 <= 1 is required", lambda: fm.ld_clump(V, p, p1=0.5, p2=0.1, samples=[7]))
    refused("p1, p2 and r2 must not be NaN", lambda: fm.ld_clump(V, p, r2=math.nan))
    refused("r2 must be within [0, 1]", lambda: fm.ld_clump(V, p, r2=1.5))
    refused("window must be within 0 .. 2^32 - 1", lambda: fm.ld_clump(V, p, window=-1))
    refused("sample 7 is outside the variants' 3 samples", lambda: fm.ld_clump(V, p[:2], samples=[7]))
    refused("sites has 4 entries for 5 rows", lambda: fm.ld_clump(V, p[:2], sites=np.ones(4, dtype=bool)))
    refused("p_values has 2 entries for 5 rows", lambda: fm.ld_clump(V, p[:2]))
    refused("p_values must be a one-dimensional float array", lambda: fm.ld_clump(V, np.zeros((5, 1))))
    refused("p value 1.500000 of row 3 is neither NaN nor within [0, 1]", lambda: fm.ld_clump(V, np.array([0.5, 0.2, np.nan, 1.5, 0.3])))
    down = [dict(position=q, genotypes=[[0, 0], [0, 0]]) for q in (10, 30, 20)]
    refused("the positions descend at variant 2: clumping needs them in order", lambda: fm.ld_clump(down, np.zeros(3)))
    refused("at least one sample is required for LD clumping", lambda: fm.ld_clump(V, p, samples=[]))
    # genotype_ld: no pair needs no device; rows are checked against the rows in play
    r2, counts = fm.genotype_ld(V, [], [], counts=True)
    assert r2.dtype == np.float64 and r2.shape == (0,) and counts.dtype == np.int64 and counts.shape == (0, 6)
    assert fm.genotype_ld(V, [], []).shape == (0,)
    refused("rows_b has 1 entries, expected 2", lambda: fm.genotype_ld(V, [0, 1], [1]))
    refused("pair 1 names rows (1, 5) of 5 rows in play", lambda: fm.genotype_ld(V, [0, 1], [1, 5]))


def test_twin_under_sanitizers(dev):
    program = os.path.join(BIN_DIR, "clump_host_check.asan")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    owned_total = 0
    for seed, K, n, prm in ((5, 300, 37, R.params(0.01, 0.1, 0.3, 60)), (9, 129, 17, R.params(0.05, 0.05, 0.0, 3)), (2, 64, 1, R.params(0.1, 0.1, 1.0, 0)),
                            (3, 1, 5, R.params(1.0, 1.0, 0.5, 0))):
        d, x, p = R.splitmix_cohort(seed, K, n)
        ref = R.clump(d, x, p, prm)
        h, owned = R.checksum(d, ref)
        owned_total += owned
        args = [seed, K, n, repr(prm["p1"]), repr(prm["p2"]), repr(prm["r2"]), prm["window"]]
        res = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        want = "clump_host_check: %d rows x %d samples, %d clumps, %d owned, checksum %016x\n" % (K, n, ref["n_clumps"], owned, h)
        assert res.stdout == want, (res.stdout, want)
    assert owned_total > 100
