"""The logistic association scan without a GPU: the library's host functions (fmh_logistic_null, fmh_logistic_score_host,
fmh_logistic_stats, ferromic.LogisticScan.from_sums) against tests/logistic_ref.py - integers with array_equal, doubles bitwise, NaN
positions equal -, the DEFINITION against dense algebra on the unquantised floats, and the p-value against scipy's chi-square tail.

Bounds.  Each is 16 x the value measured on this file's seeded set, rounded up to a power of ten (the margin tests/test_qc_cpu.py uses);
the tests print what they measure.
  Against the dense reference (a numpy Newton fit to a gradient below 1e-12, numpy.linalg.solve), over n = 64, 200, 1 000, c = 0, 1, 5, case
    fractions 0.5 and 0.1, 5 % missing: measured worst |U - U_ref| / sqrt(V_ref) = 7.7e-8 (16 x = 1.2e-6: 1e-5 is asserted) and
    |V - V_ref| / V_ref = 1.4e-8 (16 x = 2.3e-7: 1e-6 is asserted).  Both are the fixed-point quantisation of the value columns, not the fit:
    the worst cases are all c = 0, where r = y - mu takes two values only and every case (and every control) is rounded the same way, so
    the error of U adds up over the samples instead of averaging out (3.4e-8 to 7.7e-8 at n = 1 000, 1.3e-8 to 3.9e-8 at n = 200); with a
    covariate in the model the columns vary and the worst is 6.5e-9 (U) and 8.3e-9 (V).
  The p-value against scipy.stats.chi2.sf(chi2, 1) over chi2 from 0 to 1 400 (p down to 1e-306): measured worst relative error 1.9e-13
    (16 x = 3.0e-12: 1e-11 is asserted)."""

import ctypes as C

import numpy as np
import pytest

from tests import assoc_ref as A
from tests import logistic_ref as R

DENSE_U_BOUND = 1e-5
DENSE_V_BOUND = 1e-6
P_BOUND = 1e-11


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def lib():
    from ferromic_amd import _abi

    return _abi.load()


def assert_bitwise(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    assert R.same_f64(got, ref), (what, got.reshape(-1)[:4], ref.reshape(-1)[:4])


def model_inputs(n, c_in, P, seed, fraction=0.3, special=False):
    """Case / control phenotypes that depend on the first covariate, and covariates with a duplicated, a constant and a summed column when
    `special` (c_in >= 5)."""
    rng = np.random.default_rng(seed)
    cov = rng.normal(size=(n, c_in)) * rng.uniform(0.5, 3.0, size=c_in) + rng.normal(size=c_in)
    if special and c_in >= 5:
        cov[:, 2] = cov[:, 0]                # duplicated
        cov[:, 3] = 7.25                     # constant
        cov[:, 4] = cov[:, 0] + cov[:, 1]    # the sum of two others
    eta = np.log(fraction / (1.0 - fraction)) + (0.5 * (cov[:, 0] - cov[:, 0].mean()) / cov[:, 0].std() if c_in else 0.0)
    y = (rng.random((n, P)) < (1.0 / (1.0 + np.exp(-eta)))[..., None]).astype(np.float64) if c_in else (rng.random((n, P)) < fraction).astype(np.float64)
    return y, (cov if c_in else None)


def assert_null_equal(got, ref, what):
    assert got.n_basis == ref["n_basis"] and got.batch == ref["batch"], what
    assert np.array_equal(got.dropped, ref["dropped"]), what
    assert np.array_equal(got.fitted, ref["fitted"]) and np.array_equal(got.reason, ref["reason"]), (what, got.reason, ref["reason"])
    assert np.array_equal(got.iterations, ref["iterations"]) and np.array_equal(got.n_cases, ref["n_cases"]), what
    assert len(got.values) == len(ref["values"]), what
    for a, b in zip(got.values, ref["values"]):
        assert a.dtype == np.int32 and np.array_equal(a, b), what
    assert np.array_equal(got.exponent, ref["exponent"]) and got.total.tolist() == ref["total"], what


# ---- fmh_logistic_null -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 200, 1000])
@pytest.mark.parametrize("c_in", [0, 1, 5])
def test_null_matches_oracle(dev, n, c_in):
    P = 3
    y, cov = model_inputs(n, c_in, P, seed=n * 10 + c_in, special=True)
    ref = R.null_model(y, cov)
    got = dev.logistic_null(y, cov)
    assert_null_equal(got, ref, (n, c_in))
    assert ref["fitted"].all() and (ref["iterations"] >= 1).all() and (ref["iterations"] < R.MAX_STEPS).all()
    if c_in == 5:
        assert got.dropped.tolist() == [False, False, True, True, True] and got.n_basis == 2
    w = got.n_basis + 3
    big = np.abs(got.values[0]).max(axis=0)
    assert big.max() <= 1 << 30 and big.min() > 1 << 29                    # every column uses the range
    assert got.values[0].shape == (n, P * w) and got.exponent.shape == (P, w)
    assert np.array_equal(got.n_cases, (y == 1.0).sum(axis=0).astype(np.uint64))


def test_null_batches_of_whole_phenotypes(dev):
    """c = 5 kept covariates: W = 8 columns per phenotype, 8 phenotypes per batch; P = 19 gives batches of 8, 8 and 3."""
    y, cov = model_inputs(120, 5, 19, seed=5)
    ref = R.null_model(y, cov)
    got = dev.logistic_null(y, cov)
    assert_null_equal(got, ref, "three batches")
    assert got.batch == 8 and [v.shape for v in got.values] == [(120, 64), (120, 64), (120, 24)] and ref["fitted"].all()


def test_unfitted_phenotypes_leave_the_others_alone(dev):
    n = 200
    y, cov = model_inputs(n, 2, 4, seed=17)
    alone = dev.logistic_null(y[:, [0, 3]], cov)
    y[:, 1] = 0.0                                   # no case
    y[:, 2] = (cov[:, 1] > 0.0).astype(np.float64)  # separated by a covariate
    ref = R.null_model(y, cov)
    got = dev.logistic_null(y, cov)
    assert_null_equal(got, ref, "unfitted")
    assert got.fitted.tolist() == [True, False, False, True]
    assert got.reason[1] == R.ONE_CLASS and got.iterations[1] == 0 and got.n_cases[1] == 0
    assert got.reason[2] in (R.NOT_CONVERGED, R.PIVOT, R.ZERO_WEIGHT) and got.reason[2] == ref["reason"][2]
    every = dev.logistic_null(np.ones((n, 1)), cov)  # no control
    assert every.reason.tolist() == [R.ONE_CLASS] and not every.fitted[0]
    w = got.n_basis + 3
    v = got.values[0]
    assert not v[:, w:3 * w].any() and not got.exponent[1:3].any() and not got.total[1:3].any()   # zeros for the unfitted ones
    # the fitted phenotypes are bit for bit what they are without the other two
    assert np.array_equal(v[:, :w], alone.values[0][:, :w]) and np.array_equal(v[:, 3 * w:], alone.values[0][:, w:])
    assert np.array_equal(got.exponent[[0, 3]], alone.exponent) and np.array_equal(got.total[[0, 3]], alone.total)
    assert np.array_equal(got.iterations[[0, 3]], alone.iterations)


def test_null_refusals(dev, lib):
    from ferromic_amd import _abi

    y, cov = model_inputs(12, 3, 2, seed=3)
    for bad in (np.nan, np.inf):
        w = cov.copy()
        w[0, 2] = bad
        with pytest.raises(Exception, match="not finite"):
            dev.logistic_null(y, w)
    for bad in (0.5, 2.0, -1.0, np.nan):
        z = y.copy()
        z[3, 1] = bad
        with pytest.raises(Exception, match="neither 0 nor 1"):
            dev.logistic_null(z)
    with pytest.raises(Exception, match="fewer samples"):       # n = 5 < c + 3 = 6
        dev.logistic_null(y[:5], cov[:5])
    rng = np.random.default_rng(4)
    with pytest.raises(Exception, match="64 value columns"):    # 62 kept + 3
        dev.logistic_null((rng.random((200, 1)) < 0.5).astype(float), rng.normal(size=(200, 62)))
    assert dev.logistic_null((rng.random((200, 1)) < 0.5).astype(float), rng.normal(size=(200, 61))).n_basis == 61   # the limit is taken
    # NULL pointers and ranges at the C-ABI
    n, P = 12, 2
    values, e, total = np.zeros(n * P * 3, np.int32), np.zeros(P * 3, np.int32), np.zeros(P * 3, np.int64)
    fitted, reason, steps, cases = np.zeros(P, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.uint64)
    c = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ptr(y), None, n, P, 0, ptr(values), ptr(e), ptr(total), ptr(fitted), ptr(reason), ptr(steps), ptr(cases), C.byref(c), None]
    assert lib.fmh_logistic_null(*good) == _abi.FMH_OK
    for i in (0, 5, 6, 7, 8, 9, 10, 11, 12):
        args = list(good)
        args[i] = None
        assert lib.fmh_logistic_null(*args) == _abi.FMH_ERR_INVALID, i
    for i, v in ((2, 0), (2, (1 << 21) + 1), (3, 0), (4, 2)):     # n == 0, n > 2^21, P == 0, covariates without a pointer
        args = list(good)
        args[i] = v
        assert lib.fmh_logistic_null(*args) == _abi.FMH_ERR_INVALID, (i, v)


# ---- fmh_logistic_score_host, fmh_logistic_stats ---------------------------------------------------------------------------------------------
def score_case(n, c_in, P, seed, rows=40):
    """Genotypes with monomorphic, all-missing and all-het rows, a model, and the oracle's sums and tracks for the first batch."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.2, 0.8, size=(rows, 1))
    x = (rng.random((rows, 2 * n)) < freq).astype(np.uint8)
    called = rng.random((rows, 2 * n)) > 0.05
    x[0] = 0                       # monomorphic reference
    x[1] = 1                       # monomorphic alternative
    called[2] = False              # N = 0
    x[3, 0::2], x[3, 1::2] = 0, 1  # all het
    called[3] = True
    called[4] = True               # nothing missing
    y, cov = model_inputs(n, c_in, P, seed + 1)
    model = R.null_model(y, cov)
    assert model["fitted"].all()
    c = model["n_basis"]
    v = model["values"][0]
    S, Cs = A.sums(x, called, v)
    H = R.homalt_sums(x, called, v[:, c + 2::c + 3])
    Pb = v.shape[1] // (c + 3)
    total = [t for row in model["total"][:Pb] for t in row]
    return x, called, y, cov, model, S, Cs, H, A.tracks(x, called), total, model["exponent"][:Pb].reshape(-1), c


@pytest.mark.parametrize("n,c_in,P", [(64, 0, 2), (200, 1, 2), (200, 5, 3)])
def test_score_and_stats_bitwise_against_oracle(dev, n, c_in, P):
    x, called, y, cov, model, S, Cs, H, trk, total, e, c = score_case(n, c_in, P, seed=n + c_in)
    # a crafted row whose variance is negative: nothing of w on the called genotypes, everything called
    S, Cs, H = S.copy(), Cs.copy(), H.copy()
    for p in range(P):
        kw = p * (c + 3) + c + 2
        S[5, kw], H[5, p] = 0, 0
        Cs[5, kw] = total[kw]
    U_ref, V_ref = R.score(S, Cs, H, *trk, total, e, c)
    U, V = dev.logistic_score_host(S, Cs, H, *trk, total, e, c)
    assert_bitwise(U, U_ref, "score")
    assert_bitwise(V, V_ref, "variance")
    assert np.isnan(U_ref[:3]).all() and np.isnan(V_ref[:3]).all()                 # monomorphic twice, N = 0: the integer rule
    assert np.isfinite(U_ref[3:]).all() and np.isfinite(V_ref[3:]).all()
    assert (np.abs(V_ref[3]) < 1e-6).all(), "all het: a constant dosage has no variance left"
    assert (V_ref[5] < 0.0).all() and (V_ref[6:] > 0.0).all()
    assert (Cs != np.array(total, dtype=np.int64)).any(), "missing calls reach the imputation term"
    assert H.any() and (H != S[:, c + 2::c + 3]).any()
    ref = R.stats(U_ref, V_ref)
    got = dev.logistic_stats(U, V)
    for name in ("chi2", "z", "p", "beta", "se"):
        assert_bitwise(got[name], ref[name], name)
        assert np.isnan(ref[name][:3]).all() and np.isnan(ref[name][5]).all() and np.isfinite(ref[name][6:]).all()
    only = dev.logistic_stats(U, V, outputs=("p",))                               # any output may be NULL
    assert_bitwise(only["p"], ref["p"], "p alone")
    nan_in = dev.logistic_stats(np.array([np.nan, 1.0, 1.0, 1.0]), np.array([1.0, np.nan, 0.0, -1.0]))
    assert all(np.isnan(t).all() for t in nan_in.values())


def test_score_and_stats_refusals(lib):
    from ferromic_amd import _abi

    rows, c, Pb = 2, 1, 2
    K = Pb * (c + 3)
    S, H, trk = np.zeros(rows * K, np.int64), np.zeros(rows * Pb, np.int64), np.ones(rows, np.uint32)
    total, e, out = np.zeros(K, np.int64), np.zeros(K, np.int32), np.zeros(rows * Pb)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ptr(S), ptr(S), ptr(H), ptr(trk), ptr(trk), ptr(trk), rows, ptr(total), ptr(e), c, Pb, ptr(out), ptr(out)]
    assert lib.fmh_logistic_score_host(*good) == _abi.FMH_OK
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 11, 12):
        args = list(good)
        args[i] = None
        assert lib.fmh_logistic_score_host(*args) == _abi.FMH_ERR_INVALID, i
    for i, v in ((10, 0), (10, 17), (9, 62)):                     # Pb == 0, Pb (c + 3) > 64, c + 3 > 64
        args = list(good)
        args[i] = v
        assert lib.fmh_logistic_score_host(*args) == _abi.FMH_ERR_INVALID, (i, v)
    args = list(good)
    args[6], args[0] = 0, None
    assert lib.fmh_logistic_score_host(*args) == _abi.FMH_OK      # no rows: nothing is read
    u = np.ones(3)
    assert lib.fmh_logistic_stats(ptr(u), ptr(u), 3, None, None, None, None, None) == _abi.FMH_OK
    assert lib.fmh_logistic_stats(None, ptr(u), 3, None, None, None, None, None) == _abi.FMH_ERR_INVALID
    assert lib.fmh_logistic_stats(ptr(u), None, 3, None, None, None, None, None) == _abi.FMH_ERR_INVALID
    assert lib.fmh_logistic_stats(None, None, 0, None, None, None, None, None) == _abi.FMH_OK


# ---- the definition against dense algebra ----------------------------------------------------------------------------------------------------
def test_definition_against_dense_algebra(dev, capsys):
    worst_u = worst_v = 0.0
    for n in (64, 200, 1000):
        for c_in in (0, 1, 5):
            for fraction in (0.5, 0.1):
                rng = np.random.default_rng(2000 + n + 10 * c_in + int(100 * fraction))
                rows = 12
                freq = rng.uniform(0.2, 0.8, size=(rows, 1))
                x = (rng.random((rows, 2 * n)) < freq).astype(np.uint8)
                called = np.repeat(rng.random((rows, n)) > 0.05, 2, axis=1)
                cov = rng.normal(size=(n, c_in)) if c_in else None
                cg, g = A.genotypes(x, called)
                eta = np.log(fraction / (1.0 - fraction)) + 0.6 * (g[5] - g[5].mean()) + (0.3 * cov[:, 0] if c_in else 0.0)
                y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
                model = dev.logistic_null(y, cov)
                assert model.fitted.all(), (n, c_in, fraction, model.reason)
                c = model.n_basis
                v = model.values[0]
                S, Cs = A.sums(x, called, v)
                H = R.homalt_sums(x, called, v[:, c + 2:])
                trk = A.tracks(x, called)
                U, V = dev.logistic_score_host(S, Cs, H, *trk, model.total.reshape(-1), model.exponent.reshape(-1), c)
                case_u = case_v = 0.0
                for r in range(rows):
                    mu = g[r].sum() / cg[r].sum()
                    dosage = np.where(cg[r] == 1, g[r].astype(np.float64), mu)
                    U_ref, V_ref = R.dense_reference(dosage, y, cov)
                    du, dv = abs(U[r, 0] - U_ref) / np.sqrt(V_ref), abs(V[r, 0] - V_ref) / V_ref
                    case_u, case_v = max(case_u, du), max(case_v, dv)
                with capsys.disabled():
                    print(f"\nlogistic vs dense algebra: n={n} c={c_in} cases={int(y.sum())}: dU = {case_u:.3e}, dV = {case_v:.3e}", end="")
                assert case_u <= DENSE_U_BOUND and case_v <= DENSE_V_BOUND, (n, c_in, fraction, case_u, case_v)
                worst_u, worst_v = max(worst_u, case_u), max(worst_v, case_v)
    with capsys.disabled():
        print(f"\nlogistic vs dense algebra: worst |U - ref| / sqrt(V) = {worst_u:.3e}, worst |V - ref| / V = {worst_v:.3e}")


# ---- the p-value -----------------------------------------------------------------------------------------------------------------------------
def test_p_value_against_scipy(dev, capsys):
    sps = pytest.importorskip("scipy.stats")
    chi2 = np.concatenate([[0.0, 1e-300, 1e-12, 1e-6], np.linspace(0.01, 1400.0, 2000)])
    got = dev.logistic_stats(np.sqrt(chi2), np.ones_like(chi2))     # U = sqrt(chi2), Vr = 1
    ref_loop = R.stats(np.sqrt(chi2), np.ones_like(chi2))
    assert R.same_f64(got["p"], ref_loop["p"]) and got["p"][0] == 1.0
    seen = got["chi2"]                                                # the chi2 the library itself reports
    assert np.allclose(seen, chi2, rtol=1e-14, atol=0.0) and seen.max() >= 1399.9
    ref = sps.chi2.sf(seen, 1)
    assert (ref > 0.0).all() and ref.min() < 1e-300
    rel = np.abs(got["p"] - ref) / ref
    with capsys.disabled():
        print(f"\nlogistic p-value (fmh_logistic_stats) vs scipy chi2.sf: worst relative error {rel.max():.3e} at chi2 = {seen[rel.argmax()]:.3f}")
    assert (rel <= P_BOUND).all(), (seen[rel.argmax()], got["p"][rel.argmax()], ref[rel.argmax()])


# ---- ferromic.LogisticScan.from_sums -------------------------------------------------------------------------------------------------------
def test_from_sums_round_trip():
    import ferromic as fm

    n, c_in, P = 200, 5, 11                              # c = 5: two batches of 8 and 3
    rng = np.random.default_rng(91)
    rows = 30
    x = (rng.random((rows, 2 * n)) < rng.uniform(0.2, 0.8, size=(rows, 1))).astype(np.uint8)
    called = rng.random((rows, 2 * n)) > 0.05
    x[0], called[1] = 0, False
    y, cov = model_inputs(n, c_in, P, seed=92)
    y[:, 4] = 0.0                                        # not fitted
    ref = R.scan(x, called, y, cov)
    model = ref["model"]
    c, W = model["n_basis"], model["n_basis"] + 3
    assert model["fitted"].tolist() == [True] * 4 + [False] + [True] * 6 and len(model["values"]) == 2
    values = np.concatenate(model["values"], axis=1)     # [n][P * W]: the batches side by side
    S, Cs = A.sums(x, called, values)
    H = R.homalt_sums(x, called, values[:, c + 2::W])
    positions = np.arange(rows, dtype=np.int64) * 10 + 3
    kept = np.flatnonzero(~model["dropped"])
    scan = fm.LogisticScan.from_sums(S, Cs, H, *ref["tracks"], np.array(model["total"], dtype=np.int64), model["exponent"], n, c,
                                     fitted=model["fitted"], n_cases=model["n_cases"], iterations=model["iterations"], positions=positions,
                                     covariates_kept=kept, covariates_dropped=np.flatnonzero(model["dropped"]))
    assert len(scan) == rows
    for name in ("score", "variance", "chi2", "z", "p", "beta", "se"):
        assert_bitwise(getattr(scan, name), ref[name], name)
        assert np.isnan(ref[name][:, 4]).all() and np.isnan(ref[name][:2]).all() and np.isfinite(ref[name][2:, :4]).all()
    trk = ref["tracks"]
    N = trk[0].astype(np.int64) + trk[1] + trk[2]
    assert np.array_equal(scan.n_called, N.astype(np.uint32))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert R.same_f64(scan.alt_frequency, (trk[1].astype(np.float64) + 2.0 * trk[2]) / (2.0 * N))
    assert np.array_equal(scan.positions, positions) and np.array_equal(scan.covariates_kept, kept) and scan.covariates_dropped.size == 0
    assert scan.fitted.dtype == np.bool_ and np.array_equal(scan.fitted, model["fitted"])
    assert np.array_equal(scan.n_cases, model["n_cases"]) and np.array_equal(scan.iterations, model["iterations"])
    assert "LogisticScan(samples=200, sites=30, phenotypes=11, fitted=10, covariates=5)" == repr(scan)
    with pytest.raises(ValueError):
        fm.LogisticScan.from_sums(S[:3], Cs, H, *trk, np.array(model["total"], dtype=np.int64), model["exponent"], n, c)
    with pytest.raises(ValueError):
        fm.LogisticScan.from_sums(S, Cs, H[:, :3], *trk, np.array(model["total"], dtype=np.int64), model["exponent"], n, c)
