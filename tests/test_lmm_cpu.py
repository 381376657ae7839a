"""The mixed-model scan without a device: the library's host functions (fmh_lmm_projections_host, fmh_lmm_null, fmh_lmm_stats) against
tests/lmm_ref.py - the twin within the derived summation bound (tests/test_gpu_lmm.py states it), the null fit against the oracle's loops,
the statistics against a dense generalised-least-squares reference that shares no algebra with the rotation, the fixed-effects limit against
AssociationScan.from_sums, the NaN rules, every refusal in order, MixedModelScan.from_projections, and the host arithmetic under ASan and
UBSan (ferromic_amd/csrc/lmm_host_check.cpp), whose lines are compared between a plain build, the sanitizer build and the oracle.

The oracle's null fit runs the header's operation order on Python floats with the C library's log and pow, so it reproduces the library's
log10 delta bit for bit on this platform; the test asserts the 1e-9 the definition asks for."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import assoc_ref
from tests import lmm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.path.join(ROOT, "ferromic_amd", "bin")
CSRC = os.path.join(ROOT, "ferromic_amd", "csrc")


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


def covariates_of(n, count, seed):
    """`count` covariate columns; with five, column 3 is a combination of columns 0 and 1 (dropped by the basis)."""
    if count == 0:
        return None
    rng = np.random.default_rng(seed)
    cov = rng.normal(size=(n, count)) + 2.0
    if count >= 5:
        cov[:, 3] = 0.5 * cov[:, 0] - 2.0 * cov[:, 1] + 1.0
    return cov


def eigen_of(A):
    w, u = np.linalg.eigh(A)
    order = np.argsort(-w, kind="stable")
    return w[order], np.ascontiguousarray(u[:, order])


def phenotypes_of(code, A, P, seed):
    """Phenotypes with a polygenic part (so that delta is interior for the first) and noise."""
    rng = np.random.default_rng(seed)
    n = code.shape[1]
    w, u = eigen_of(A)
    g = u @ (np.sqrt(np.maximum(w, 0.0)) * rng.normal(size=n))
    y = np.stack([(1.5 * g if p % 2 == 0 else 0.2 * g) + rng.normal(size=n) + 3.0 for p in range(P)], axis=1)
    return y


# ---- 1. the twin against the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,P,L", [(1, 1, 1, 1), (17, 5, 16, 64), (70, 70, 2, 17)])
def test_twin_against_oracle(dev, n, K, P, L):
    rng = np.random.default_rng(n + K)
    code = R.related_codes(40, n, seed=3, missing=0.1)
    basis, weights, linear = rng.normal(size=(n, K)), rng.uniform(0, 2, size=(P, K)), rng.normal(size=(L, K))
    ref = R.projections(code, basis, weights, linear)
    got = dev.lmm_projections_host(code, basis, weights, linear)
    assert np.array_equal(got.called, ref["c"]) and np.array_equal(got.allele_count, ref["a"])
    wq, wl = R.worst_ratio(got.quad, ref["quad"], ref["quad_bound"]), R.worst_ratio(got.lin, ref["lin"], ref["lin_bound"])
    print(f"twin n={n} K={K}: worst err / (2 bound): quad {wq:.3e}, lin {wl:.3e}")
    assert wq <= 1.0 and wl <= 1.0
    if n <= 17:  # and bit for bit the plain loops
        quad, lin = R.twin(code, basis, weights, linear)
        assert assoc_ref.same_f64(got.quad, quad) and assoc_ref.same_f64(got.lin, lin)


# ---- 2. the null fit against the oracle's loops -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,covs", [(64, 0), (64, 5), (120, 1)])
def test_null_fit_against_oracle(dev, n, covs):
    code = R.related_codes(300, n, seed=n + covs)
    A = R.grm_of(code)
    w, u = eigen_of(A)
    y = phenotypes_of(code, A, 2, seed=5)
    cov = covariates_of(n, covs, seed=6)
    got = dev.lmm_null(w, u, y, cov)
    ref = R.null_fit(w, u, y, cov)
    assert got.q == ref["q"] and np.array_equal(got.dropped, ref["dropped"]) and (covs < 5 or list(np.flatnonzero(got.dropped)) == [3])
    assert not got.reason.any() and not ref["reason"].any()
    for p in range(2):
        assert np.all(got.log_likelihood[p] >= got.grid_log_likelihood[p]), "l at the returned delta is at least l at every grid point"
        assert np.isfinite(got.grid_log_likelihood[p]).all()
        assert abs(np.log10(got.delta[p]) - ref["log10_delta"][p]) <= 1e-9, (got.delta[p], ref["delta"][p])
        print(f"null n={n} covs={covs} p={p}: log10 delta {np.log10(got.delta[p]):.6f}, h2 {got.heritability[p]:.4f}, boundary {got.at_boundary[p]}")
    assert np.array_equal(got.at_boundary, ref["at_boundary"])
    for name in ("sigma_g2", "sigma_e2", "heritability", "log_likelihood", "R"):
        assert np.allclose(getattr(got, name), ref[name], rtol=1e-9, atol=0), name
    assert np.allclose(got.grid_log_likelihood, ref["grid"], rtol=1e-12, atol=1e-9)
    assert np.allclose(got.weights, ref["weights"], rtol=1e-9, atol=0) and np.allclose(got.linear, ref["linear"], rtol=1e-9, atol=1e-300)
    assert np.allclose(got.M, ref["M"], rtol=1e-8, atol=1e-300) and np.allclose(got.v, ref["v"], rtol=1e-8, atol=1e-14)
    assert 1e-5 < got.delta[0] < 1e5 and not got.at_boundary[0], "the first phenotype has an interior delta"
    # a fixed delta skips the search, bit for bit the oracle's
    fixed = dev.lmm_null(w, u, y, cov, fixed_delta=[0.5, 2.0])
    fref = R.null_fit(w, u, y, cov, fixed_delta=[0.5, 2.0])
    for name in ("weights", "linear", "M", "v", "R"):
        assert assoc_ref.same_f64(getattr(fixed, name), fref[name]), name
    assert list(fixed.delta) == [0.5, 2.0] and not fixed.at_boundary.any()


# ---- 3. the statistics against the dense reference at the library's delta ------------------------------------------------------------------------
@pytest.mark.parametrize("n,covs", [(64, 0), (64, 5), (200, 1), (200, 5), (500, 0), (500, 5)])
def test_statistics_against_dense_reference(dev, n, covs):
    code = R.related_codes(400, n, seed=2 * n + covs, missing=0.05)
    A = R.grm_of(code)
    assert np.abs(A - np.eye(n) * A[0, 0]).max() > 0.3, "relatives: A is far from a multiple of the identity"
    w, u = eigen_of(A)
    y = phenotypes_of(code, A, 2, seed=7)
    cov = covariates_of(n, covs, seed=8)
    fit = dev.lmm_null(w, u, y, cov)
    scan = code[:40]
    got = dev.lmm_projections_host(scan, u, fit.weights, fit.linear)
    st = dev.lmm_stats(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
    kept = None if cov is None else cov[:, ~fit.dropped]
    worst_beta = worst_t = 0.0
    for p in range(2):
        ref = R.dense(scan, A, fit.delta[p], y[:, p], kept)
        ok = np.isfinite(ref["beta"])
        assert np.array_equal(ok, np.isfinite(st["beta"][:, p])) and ok.sum() >= 30 and not ok[:3].any()
        worst_beta = max(worst_beta, float((np.abs(st["beta"][ok, p] - ref["beta"][ok]) / ref["se"][ok]).max()))
        worst_t = max(worst_t, float((np.abs(st["t"][ok, p] - ref["t"][ok]) / np.maximum(1.0, np.abs(ref["t"][ok]))).max()))
        assert np.all(np.abs(st["se"][ok, p] - ref["se"][ok]) <= 1e-6 * ref["se"][ok])
        tails = np.array([assoc_ref.student_t_two_sided(t, n - fit.q - 1) for t in st["t"][ok, p]])
        assert np.all(np.abs(st["p"][ok, p] - tails) <= 1e-9 * tails + 1e-300)
    print(f"dense n={n} covs={covs}: worst |beta - ref| / se {worst_beta:.3e}, worst |t - ref| / max(1, |t|) {worst_t:.3e}")
    assert worst_beta <= 1e-6 and worst_t <= 1e-6


# ---- 4. the fixed-effects limit -------------------------------------------------------------------------------------------------------------------
def alleles_of(code):
    """x [rows][2 n] alleles and called flags of a code table."""
    x = np.zeros((code.shape[0], 2 * code.shape[1]), dtype=np.uint8)
    x[:, 0::2] = code >= 1
    x[:, 1::2] = code == 2
    called = np.repeat(code <= 2, 2, axis=1)
    return np.where(called, x, 0).astype(np.uint8), called


@pytest.mark.parametrize("covs", [0, 3])
def test_fixed_effects_limit(dev, fm, covs):
    """A = I: V = (1 + delta) I, generalised least squares is least squares whatever delta is."""
    n = 90
    code = R.related_codes(80, n, seed=11)
    y = np.random.default_rng(12).normal(size=(n, 2)) + 1.0
    cov = covariates_of(n, covs, seed=13)
    x, called = alleles_of(code)
    prep = assoc_ref.prepare(y, cov)
    S, Cs = assoc_ref.sums(x, called, prep["values"], None)
    trk = assoc_ref.tracks(x, called, None)
    fixed = fm.AssociationScan.from_sums(S, Cs, *trk, np.array(prep["total"], dtype=np.int64), prep["exponent"], prep["yy"], n, prep["n_basis"])
    assert fixed.df == n - covs - 2
    for delta in (0.01, 1.0, 100.0):
        fit = dev.lmm_null(np.ones(n), np.eye(n), y, cov, fixed_delta=[delta, delta])
        got = dev.lmm_projections_host(code, np.eye(n), fit.weights, fit.linear)
        st = dev.lmm_stats(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
        for name in ("beta", "se", "t", "p"):
            want = getattr(fixed, name)
            ok = np.isfinite(want)
            assert np.array_equal(ok, np.isfinite(st[name])) and ok.sum() > 100, name
            assert np.all(np.abs(st[name][ok] - want[ok]) <= 1e-6 * np.maximum(1.0, np.abs(want[ok]))), (name, delta)


# ---- 5. the NaN rules -----------------------------------------------------------------------------------------------------------------------------
def test_nan_rules(dev):
    n = 30
    code = R.related_codes(20, n, seed=14)
    code[5] = np.where(code[5] == 3, 3, 2)  # monomorphic among the called
    A = R.grm_of(R.related_codes(200, n, seed=15))
    w, u = eigen_of(A)
    rng = np.random.default_rng(16)
    y = np.stack([rng.normal(size=n), np.full(n, 0.1), rng.normal(size=n)], axis=1)  # the second phenotype is constant
    fit = dev.lmm_null(w, u, y, None)
    assert list(fit.reason) == [0, 1, 0] and np.isnan(fit.delta[1]) and np.isnan(fit.M[1]).all() and not fit.weights[1].any() and not fit.at_boundary[1]
    got = dev.lmm_projections_host(code, u, fit.weights, fit.linear)
    st = dev.lmm_stats(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
    c, a = R.counts(code)
    polymorphic = (c > 0) & (a > 0) & (a < 2 * c)
    live = np.flatnonzero(polymorphic)
    assert not polymorphic[[0, 1, 2, 5]].any() and live.size >= 10
    for name in ("beta", "se", "t", "p"):
        assert np.isnan(st[name][:, 1]).all(), "a constant phenotype: NaN columns"
        assert np.isnan(st[name][[0, 1, 2, 5]]).all(), "all hom-ref, all uncalled, all hom-alt, monomorphic among the called"
        assert np.array_equal(np.isfinite(st[name][:, 0]), polymorphic) and np.array_equal(np.isfinite(st[name][:, 2]), polymorphic)
    # not D > 0: a quad entry at or below a^T M a
    quad, lin = got.quad.copy(), got.lin
    r7, r8 = live[0], live[1]
    quad[r7, 0] = 0.0
    quad[r8, 2] = np.nan
    st2 = dev.lmm_stats(quad, lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
    assert np.isnan([st2[k][r7, 0] for k in st2]).all() and np.isnan([st2[k][r8, 2] for k in st2]).all() and np.isfinite(st2["beta"][r7, 2])
    # se == 0: t and p are NaN, beta and se are not
    R0 = fit.R.copy()
    R0[0] = 0.0
    st3 = dev.lmm_stats(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, R0, n)
    assert np.all(st3["se"][live, 0] == 0.0) and np.isfinite(st3["beta"][live, 0]).all() and np.isnan(st3["t"][live, 0]).all() and np.isnan(st3["p"][live, 0]).all()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order(dev):
    from ferromic_amd import _abi as abi

    lib = abi.load()
    n, P = 12, 2
    rng = np.random.default_rng(17)
    lam, U, Y, cov = np.abs(rng.normal(size=n)), np.eye(n), rng.normal(size=(n, P)), rng.normal(size=(n, 2))
    f = lambda *shape: np.zeros(shape)
    arrays = [f(P), f(P), f(P), f(P), f(P), np.zeros(P, np.uint8), np.zeros(P, np.uint8), f(P * n), f(P * 4 * n), f(P * 9), f(P * 3), f(P), None]
    out = abi.LmmNullOut(*(None if a is None else a.ctypes.data for a in arrays))
    q, dropped = C.c_size_t(0), np.zeros(2, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def null(lam=lam, U=U, Y=Y, cov=cov, n=n, P=P, cin=2, fixed=None, q=q, o=out):
        return lib.fmh_lmm_null(p(lam), p(U), p(Y), p(cov), n, P, cin, p(fixed), None if q is None else C.byref(q), p(dropped), None if o is None else C.byref(o))

    bad_out = abi.LmmNullOut(*(None if i == 7 or a is None else a.ctypes.data for i, a in enumerate(arrays)))
    nan_y, inf_cov, nan_lam = Y.copy(), cov.copy(), lam.copy()
    nan_y[3, 1], inf_cov[0, 0], nan_lam[2] = np.nan, np.inf, np.nan
    invalid = [null(lam=None), null(U=None), null(Y=None), null(q=None), null(o=None), null(o=bad_out), null(cov=None), null(P=0), null(n=0), null(lam=nan_lam),
               null(Y=nan_y), null(cov=inf_cov), null(fixed=np.array([1.0, 0.0])), null(fixed=np.array([np.nan, 1.0]))]
    assert invalid == [abi.FMH_ERR_INVALID] * len(invalid), invalid
    assert null(Y=nan_y, n=4) == abi.FMH_ERR_INVALID and b"not finite" in lib.fmh_last_error()  # a non-finite input before the degrees of freedom
    assert null(n=4) == abi.FMH_ERR_INVALID and b"degrees of freedom" in lib.fmh_last_error()   # q = 3: n - q - 1 = 0
    assert null(n=5) == 0 and q.value == 3
    wide_y, wide_out = rng.normal(size=(n, 17)), None
    big = [f(17), f(17), f(17), f(17), f(17), np.zeros(17, np.uint8), np.zeros(17, np.uint8), f(17 * n), f(17 * 4 * n), f(17 * 9), f(17 * 3), f(17), None]
    wide_out = abi.LmmNullOut(*(None if a is None else a.ctypes.data for a in big))
    assert null(Y=wide_y, P=17, o=wide_out) == abi.FMH_ERR_INVALID and b"P <= 16" in lib.fmh_last_error()
    assert null(Y=wide_y, P=16, o=wide_out) == 0  # 16 * 4 = 64 coefficient rows
    assert null(Y=wide_y, P=16, o=wide_out, n=4) == abi.FMH_ERR_INVALID and b"degrees of freedom" in lib.fmh_last_error()  # before the batch limit

    d = f(8)
    c32 = np.zeros(4, np.uint32)
    stats = lambda rows=2, n=10, q=1, P=1, quad=d: lib.fmh_lmm_stats(p(quad), p(d), p(c32), p(c32), rows, p(d), p(d), p(d), n, q, P, p(d), p(d), p(d), p(d))
    assert [stats(P=0), stats(P=17), stats(q=0), stats(q=32, P=2, n=99), stats(n=2), stats(quad=None)] == [abi.FMH_ERR_INVALID] * 6
    assert stats(rows=0, quad=None) == 0 and stats() == 0
    host = lambda rows=1, n=2, K=2, P=1, L=1, dos=np.zeros(4, np.uint8), b=d: lib.fmh_lmm_projections_host(p(dos), rows, n, p(b), K, p(d), P, p(d), L, p(d), p(d), None, None)
    assert [host(b=None), host(dos=None), host(n=0), host(K=0), host(K=32769), host(P=17), host(L=65)] == [abi.FMH_ERR_INVALID] * 7
    assert host() == 0 and host(rows=0, dos=None) == 0
    assert lib.fmh_lmm_projections(None, None, 1, 0, 0, p(d), 1, p(d), 1, p(d), 1, p(d), p(d), None, None, None) == abi.FMH_ERR_INVALID


def test_python_argument_errors_need_no_device(fm):
    variants = [dict(position=10 + i, genotypes=[[0, 1], [1, 1], [0, 0], [0, 1], None, [1, 0]]) for i in range(8)]
    y, eye = np.arange(6.0), np.eye(6)
    bad = [dict(phenotypes=np.arange(5.0), relationship=eye), dict(phenotypes=y, relationship=np.eye(5)), dict(phenotypes=y, relationship=eye + np.triu(np.ones((6, 6)), 1)),
           dict(phenotypes=y, relationship=eye, covariates=np.ones((5, 1))), dict(phenotypes=y, relationship=eye, covariates=np.ones(6)),
           dict(phenotypes=np.where(y == 2, np.nan, y), relationship=eye), dict(phenotypes=y, relationship=eye, eigen=(np.ones(5), eye)),
           dict(phenotypes=y, relationship=eye, eigen=eye), dict(phenotypes=y, relationship=eye, samples=[3, 1]), dict(phenotypes=np.zeros((6, 0)), relationship=eye),
           dict(phenotypes=y, relationship=eye, covariates=np.ones((6, 63)))]
    for kw in bad:
        with pytest.raises(ValueError):
            fm.mixed_model_scan(variants, **kw)


# ---- 7. from_projections ----------------------------------------------------------------------------------------------------------------------------
def test_from_projections(dev, fm):
    n = 40
    code = R.related_codes(60, n, seed=18)
    A = R.grm_of(R.related_codes(300, n, seed=19))
    w, u = eigen_of(A)
    y = phenotypes_of(code, A, 3, seed=20)
    cov = covariates_of(n, 5, seed=21)
    fit = dev.lmm_null(w, u, y, cov)
    got = dev.lmm_projections_host(code, u, fit.weights, fit.linear)
    st = dev.lmm_stats(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
    positions = np.arange(60, dtype=np.int64) * 7 + 1
    scan = fm.MixedModelScan.from_projections(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n, positions=positions, delta=fit.delta,
                                              covariates_kept=np.flatnonzero(~fit.dropped), covariates_dropped=np.flatnonzero(fit.dropped), eigenvalues=w)
    for name in ("beta", "se", "t", "p"):
        assert assoc_ref.same_f64(getattr(scan, name), st[name]), name
    assert len(scan) == 60 and scan.df == n - fit.q - 1 and "MixedModelScan(samples=40, sites=60, phenotypes=3, covariates=4" in repr(scan)
    assert np.array_equal(scan.n_called, got.called) and np.array_equal(scan.positions, positions) and list(scan.covariates_dropped) == [3]
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(scan.alt_frequency, got.allele_count / (2.0 * got.called), equal_nan=True)
    assert np.array_equal(scan.delta, fit.delta) and np.array_equal(scan.heritability, 1.0 / (1.0 + fit.delta)) and np.array_equal(scan.eigenvalues, w)
    with pytest.raises(ValueError):
        fm.MixedModelScan.from_projections(got.quad[:5], got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, n)
    with pytest.raises(ValueError):
        fm.MixedModelScan.from_projections(got.quad, got.lin, got.called, got.allele_count, fit.M, fit.v, fit.R, fit.q + 1)


# ---- 8. the host arithmetic under ASan + UBSan ----------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(dev, tmp_path):
    program = os.path.join(BIN_DIR, "lmm_host_check.asan")
    res = subprocess.run(["make", "-C", CSRC, program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    plain = str(tmp_path / "lmm_host_check")
    res = subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-std=c++17", "-o", plain, os.path.join(CSRC, "lmm_host_check.cpp")],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    seen_flat = seen_fit = False
    for seed, rows, n, flat in [(1, 40, 12, 0), (2, 30, 9, 1), (3, 1, 8, 0), (4, 70, 21, 0)]:
        outs = []
        for binary in (plain, program):
            res = subprocess.run([binary, str(seed), str(rows), str(n), str(flat)], capture_output=True, text=True, timeout=300, env=env)
            assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
            outs.append(res.stdout)
        assert outs[0] == outs[1], outs
        line, deltas = R.check_lines(seed, rows, n, flat)
        got_line, got_delta = outs[1].splitlines()
        assert got_line == line, (got_line, line)
        for got, want in zip(got_delta.split()[1:], deltas):
            if np.isnan(want):
                assert "nan" in got
                seen_flat = True
            else:
                assert abs(np.log10(float(got)) - np.log10(want)) <= 1e-9, (got, want)
                seen_fit = True
    assert seen_flat and seen_fit
