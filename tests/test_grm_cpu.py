"""The genomic relationship matrix without a device: the numpy oracle (tests/grm_ref.py) against a triple loop, the library's host functions
(fmh_grm_values, fmh_grm_finish bitwise; fmh_grm_host within the summation bound) against the oracle, known answers, the argument refusals of
the Python surface, and the host arithmetic under ASan and UBSan (ferromic_amd/csrc/grm_host_check.cpp), whose checksum line is compared
with the oracle's over a splitmix64 cohort that tests/grm_ref.py restates."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import grm_ref as R

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


def random_codes(K, n, seed, miss=0.05):
    rng = np.random.default_rng(seed)
    freq = rng.beta(0.5, 0.5, size=(K, 1))
    code = ((rng.random((K, n)) < freq).astype(np.uint8) + (rng.random((K, n)) < freq).astype(np.uint8)).astype(np.uint8)
    code[rng.random((K, n)) < miss] = 3
    return code


def special_codes(n=9, seed=2):
    """Random rows plus the edge rows: monomorphic (all hom-ref, all hom-alt), all missing, one called sample (het, and hom-ref)."""
    code = random_codes(40, n, seed, miss=0.2)
    code[0] = 0
    code[1] = 2
    code[2] = 3
    code[3] = 3
    code[3, 4] = 1   # one called sample, het: c = 1, a = 1: usable, p = 0.5
    code[5] = 3
    code[5, 0] = 0   # one called sample, hom-ref: not usable
    code[6, :] = np.where(code[6] == 3, 3, 2)  # monomorphic among the called
    return code


# ---- 1. the oracle against a triple loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_oracle_against_brute_force(method):
    code = special_codes()
    S, absprod, Z, usable, z, scale, m = R.products(code, method)
    Sb, Nb = R.brute(code, method)
    assert 0 < m < code.shape[0] and not usable[0] and not usable[1] and not usable[2] and usable[3] and not usable[5] and not usable[6]
    assert np.all(np.abs(S - Sb) <= R.bound(absprod, m))
    assert np.array_equal(R.pair_sites(code, usable), Nb)
    assert np.array_equal(S, S.T)


# ---- 2. values and finish, bitwise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_values_and_finish_bitwise(dev, method):
    code = special_codes(n=11, seed=4)
    code[:, 10] = np.where(np.arange(code.shape[0]) % 2 == 0, 3, code[:, 10])
    code[:, 9] = np.where(np.arange(code.shape[0]) % 2 == 1, 3, code[:, 9])  # samples 9 and 10 share no called row: N = 0
    c, a = R.counts(code)
    usable, p, z, scale, m = R.values(c, a, method)
    g_usable, g_p, g_z, g_scale, g_m = dev.grm_values(c, a, method)
    assert np.array_equal(g_usable, usable) and g_m == m
    assert np.array_equal(g_p.view(np.uint64)[c > 0], p.view(np.uint64)[c > 0]) and np.isnan(g_p[c == 0]).all() and (c == 0).any()
    assert np.array_equal(g_z.view(np.uint64), z.view(np.uint64))
    assert np.float64(g_scale).view(np.uint64) == np.float64(scale).view(np.uint64)
    S = R.products(code, method)[0]
    N = R.pair_sites(code, usable)
    assert N[9, 10] == 0 and N[10, 9] == 0
    for denominator in ("sites", "pairs") if method == "standardized" else ("sites",):
        A = R.matrix(S, N, method, denominator, m, scale)
        got = dev.grm_finish(S, N if denominator == "pairs" else None, m, scale, dev.grm_params(method, denominator))
        assert np.array_equal(np.isnan(got), np.isnan(A)), denominator
        assert np.array_equal(got.view(np.uint64)[~np.isnan(A)], A.view(np.uint64)[~np.isnan(A)]), denominator
        if denominator == "pairs":
            assert np.isnan(got[9, 10]) and np.isnan(got[10, 9]) and np.isfinite(got[0, 1])


# ---- 3. the twin within the summation bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_twin_within_the_bound(dev, method):
    code = random_codes(300, 23, 6)
    code[7] = 0
    code[8] = 3
    S, absprod, _, usable, _, scale, m = R.products(code, method)
    got_S, got_N, got_m, got_scale = dev.grm_host(code, method)
    assert got_m == m and np.float64(got_scale).view(np.uint64) == np.float64(scale).view(np.uint64)
    assert np.array_equal(got_N, R.pair_sites(code, usable))
    err, bound = np.abs(got_S - S), R.bound(absprod, m)
    print(f"twin {method}: worst err/bound {float((err / bound).max()):.3e}")
    assert np.all(err <= bound)
    assert np.array_equal(got_S, got_S.T)


# ---- 4. known answers -----------------------------------------------------------------------------------------------------------------------------
def test_known_answers(dev):
    code = random_codes(400, 12, 9, miss=0.0)
    code[:, 5] = code[:, 2]  # a duplicated sample
    S, N, m, scale = dev.grm_host(code, "standardized")
    A = dev.grm_finish(S, None, m, scale)
    assert A[2, 5] == A[2, 2] == A[5, 5]
    # complete data, standardized: every row of Z sums to 0 over the samples, so the rows of A do
    _, absprod, _, _, _, _, _ = R.products(code, "standardized")
    assert np.all(np.abs(A.sum(axis=1)) <= 12 * R.bound(absprod, m).max() / m)
    # centered with denominator sites is VanRaden's first matrix: (M - P)(M - P)^T / (2 sum p (1 - p)), M the dosages, P = 2 p
    Sc, _, mc, sc = dev.grm_host(code, "centered")
    Ac = dev.grm_finish(Sc, None, mc, sc, dev.grm_params("centered", "sites"))
    c, a = R.counts(code)
    use = (a > 0) & (a < 2 * c)
    M = code[use].astype(np.float64)
    p = M.mean(axis=1) / 2.0
    W = M - 2.0 * p[:, None]
    G = W.T @ W / (2.0 * (p * (1.0 - p)).sum())
    assert np.allclose(Ac, G, rtol=1e-12, atol=1e-12)


# ---- 5. the Python surface's refusals (no device is reached) -------------------------------------------------------------------------------------
def records(K=6, n=4):
    return [{"position": 10 * k + 1, "genotypes": [(k % 2, (k + s) % 2) for s in range(n)]} for k in range(K)]


def test_python_surface_refusals(fm):
    assert fm.GeneticRelationship.__module__.endswith("_core") and fm.GenotypePCA.__module__.endswith("_core")
    assert callable(fm.grm) and hasattr(fm.Population, "grm")
    V = records()
    with pytest.raises(ValueError, match="method"):
        fm.grm(V, method="vanraden2")
    with pytest.raises(ValueError, match="denominator"):
        fm.grm(V, denominator="rows")
    with pytest.raises(ValueError, match="pairs"):
        fm.grm(V, method="centered", denominator="pairs")
    with pytest.raises(ValueError, match="outside"):
        fm.grm(V, samples=[0, 9])
    with pytest.raises(ValueError, match="ascending"):
        fm.grm(V, samples=[2, 1])
    with pytest.raises(ValueError, match="at least one sample"):
        fm.grm(V, samples=[])
    with pytest.raises(TypeError):
        fm.grm(V, samples=["a"])
    haploid = [{"position": 1, "genotypes": [(0,), (1,)]}]
    with pytest.raises(ValueError, match="ploidy"):
        fm.grm(haploid)
    pop = fm.Population("p", V, [(0, 0), (0, 1), (1, 0), (1, 1)], 100)
    with pytest.raises(ValueError, match="method"):
        pop.grm(method="x")


def test_library_refusals(dev):
    lib, abi = dev._abi.load(), dev._abi
    c = np.array([3], dtype=np.uint32)
    assert lib.fmh_grm_values(c.ctypes.data, c.ctypes.data, 1, 7, None, None, None, None, None) == abi.FMH_ERR_INVALID
    S = np.zeros((2, 2))
    bad = abi.GrmParams(1, 1)
    assert lib.fmh_grm_finish(S.ctypes.data, None, 2, C.byref(bad), 1, 1.0, S.ctypes.data) == abi.FMH_ERR_INVALID and b"FMH_GRM_PAIRS" in lib.fmh_last_error()
    pairs = abi.GrmParams(0, 1)
    assert lib.fmh_grm_finish(S.ctypes.data, None, 2, C.byref(pairs), 1, 1.0, S.ctypes.data) == abi.FMH_ERR_INVALID
    assert lib.fmh_grm_finish(S.ctypes.data, None, 2, None, 1, 1.0, S.ctypes.data) == abi.FMH_ERR_INVALID
    assert lib.fmh_grm_host(None, 0, 0, 0, S.ctypes.data, None, None, None) == abi.FMH_ERR_INVALID
    assert lib.fmh_grm_eigen(0, None, 2, 1, S.ctypes.data, S.ctypes.data) == abi.FMH_ERR_INVALID
    assert lib.fmh_grm(None, None, 1, 0, 0, None, C.byref(pairs), None, None, None) == abi.FMH_ERR_INVALID


# ---- 6. the host arithmetic under ASan + UBSan ------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(dev):
    program = os.path.join(BIN_DIR, "grm_host_check.asan")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    usable_total = 0
    for seed, K, n, method, denominator in [(1, 90, 7, "standardized", "sites"), (2, 65, 9, "standardized", "pairs"), (3, 120, 5, "centered", "sites"),
                                            (4, 1, 3, "standardized", "sites")]:
        res = subprocess.run([program, str(seed), str(K), str(n), str(R.METHODS.index(method)), "1" if denominator == "pairs" else "0"],
                             capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        code = R.check_cohort(seed, K, n)
        h, m = R.checksum(code, method, denominator, R.brute(code, method)[0])
        usable_total += m
        want = "grm_host_check: %d rows x %d samples, %d usable, checksum %016x\n" % (K, n, m, h)
        assert res.stdout == want, (res.stdout, want)
    assert usable_total > 150
