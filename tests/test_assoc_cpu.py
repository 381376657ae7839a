"""The association scan without a GPU: the library's host functions (fmh_assoc_prepare, fmh_assoc_stats, ferromic.AssociationScan.from_sums)
against tests/assoc_ref.py - integers with array_equal, doubles bitwise -, the DEFINITION against ordinary least squares on the original
floats, and the p-value against an independent evaluation of the Student-t tail.

Bounds.  Against least squares: |beta - beta_ols| <= 1e-6 se_ols and |t - t_ols| <= 1e-6 max(1, |t_ols|).  The fixed-point quantisation
(values scaled to 2^30, an analytic intercept) measured at most 9.1e-9 on such inputs and the same formulas without quantisation 1e-12, so
1e-6 leaves two orders for other seeds.  Measured by this file's seeded set: beta 6.6e-9 se, t 6.5e-9 (printed by the test).
The p-value: relative 1e-9 against scipy; the continued fraction is iterated to 1e-15 and the lgamma differences cost a few 1e-13.  Measured
on fmh_assoc_stats' own p over this file's grid (df 1, 2, 10, 997; |t| 0 .. 40): 3.0e-13 (printed by the test)."""

import ctypes as C

import numpy as np
import pytest

from tests import assoc_ref as R


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


def model_inputs(n, c_in, P, seed, special=False):
    """Phenotypes and covariates with a duplicated, a constant and a summed covariate when `special` (c_in >= 5)."""
    rng = np.random.default_rng(seed)
    cov = rng.normal(size=(n, c_in)) * rng.uniform(0.1, 50.0, size=c_in) + rng.normal(size=c_in)
    if special and c_in >= 5:
        cov[:, 2] = cov[:, 0]                # duplicated
        cov[:, 3] = 7.25                     # constant
        cov[:, 4] = cov[:, 0] + cov[:, 1]    # the sum of two others
    y = rng.normal(size=(n, P))
    if c_in:
        y = y + cov[:, :1] * 0.3
    return y, (cov if c_in else None)


# ---- fmh_assoc_prepare ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 64, 200, 1000])
@pytest.mark.parametrize("c_in", [0, 1, 5])
@pytest.mark.parametrize("P", [1, 3])
def test_prepare_matches_oracle(dev, n, c_in, P):
    if n - min(c_in, 2) - 2 < 1:
        c_in = 0 if n == 3 else min(c_in, 1)   # the smallest cohorts keep a residual degree of freedom
    y, cov = model_inputs(n, c_in, P, seed=n * 100 + c_in * 10 + P, special=n >= 64)
    if n >= 64:
        y[:, 0] *= 1e-30                       # a tiny scale: an exponent above 60
        if P > 1:
            y[:, 1] *= 1e12                    # a huge scale: a negative exponent
    ref = R.prepare(y, cov)
    got = dev.assoc_prepare(y, cov)
    assert got.n_basis == ref["n_basis"]
    assert np.array_equal(got.dropped, ref["dropped"])
    if c_in == 5 and n >= 64:
        assert got.dropped.tolist() == [False, False, True, True, True]
    assert got.values.dtype == np.int32 and np.array_equal(got.values, ref["values"])
    assert np.array_equal(got.exponent, ref["exponent"])
    assert got.total.tolist() == ref["total"]
    assert_bitwise(got.yy, ref["yy"], "yy")
    assert np.abs(got.values).max() <= 1 << 30 and np.abs(got.values).max(axis=0).min() > 1 << 29   # every column uses the range
    if n >= 64:
        assert got.exponent[got.n_basis] > 60
        if P > 1:
            assert got.exponent[got.n_basis + 1] < 0


def test_prepare_zero_column_and_exact_power_of_two(dev):
    y = np.zeros((8, 2))
    y[:, 1] = [4, -4, 4, -4, 4, -4, 4, -4]     # centred max 4.0 = 0.5 * 2^3: the exponent is 31 - 3 = 28 and the values +-2^30
    got, ref = dev.assoc_prepare(y), R.prepare(y)
    assert got.exponent.tolist() == [0, 28] == ref["exponent"].tolist()
    assert np.array_equal(got.values, ref["values"]) and np.abs(got.values[:, 1]).max() == 1 << 30 and not got.values[:, 0].any()


def test_prepare_refusals(dev, lib):
    from ferromic_amd import _abi

    y = np.random.default_rng(1).normal(size=(10, 2))
    cov = np.random.default_rng(2).normal(size=(10, 3))
    for bad in (np.nan, np.inf):
        z = y.copy()
        z[3, 1] = bad
        with pytest.raises(Exception, match="not finite"):
            dev.assoc_prepare(z)
        w = cov.copy()
        w[0, 2] = bad
        with pytest.raises(Exception, match="not finite"):
            dev.assoc_prepare(y, w)
    with pytest.raises(Exception, match="degrees of freedom"):   # n - c - 2 = 0
        dev.assoc_prepare(y[:5], cov[:5])
    with pytest.raises(Exception, match="value columns"):        # 60 kept + 5
        dev.assoc_prepare(np.random.default_rng(3).normal(size=(200, 5)), np.random.default_rng(4).normal(size=(200, 60)))
    # NULL pointers and ranges at the C-ABI
    n, P = 10, 2
    values, e, total, yy = np.zeros(n * P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int64), np.zeros(P)
    c = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ptr(y), None, n, P, 0, ptr(values), ptr(e), ptr(total), ptr(yy), C.byref(c), None]
    assert lib.fmh_assoc_prepare(*good) == _abi.FMH_OK
    for i in (0, 5, 6, 7, 8, 9):
        args = list(good)
        args[i] = None
        assert lib.fmh_assoc_prepare(*args) == _abi.FMH_ERR_INVALID, i
    for i, v in ((2, 0), (2, (1 << 22) + 1), (3, 0), (4, 2)):     # n == 0, n > 2^22, P == 0, covariates without a pointer
        args = list(good)
        args[i] = v
        assert lib.fmh_assoc_prepare(*args) == _abi.FMH_ERR_INVALID, (i, v)


# ---- fmh_assoc_stats ------------------------------------------------------------------------------------------------------------------
def stats_case(n, c_in, P, seed, rows=40):
    """Genotypes with monomorphic, all-missing, all-het and partly missing rows, a model, and the oracle's sums and tracks."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.2, 0.8, size=(rows, 1))
    x = (rng.random((rows, 2 * n)) < freq).astype(np.uint8)
    called = rng.random((rows, 2 * n)) > 0.05
    x[0] = 0                      # monomorphic reference
    x[1] = 1                      # monomorphic alternative
    called[2] = False             # N = 0
    x[3, 0::2], x[3, 1::2] = 0, 1  # all het
    called[3] = True
    called[4] = True              # nothing missing
    y, cov = model_inputs(n, c_in, P, seed + 1)
    y[:, P - 1] = 3.5             # a constant phenotype: rss == 0, se == 0
    prep = R.prepare(y, cov)
    S, Cs = R.sums(x, called, prep["values"])
    return x, called, y, cov, prep, S, Cs, R.tracks(x, called)


@pytest.mark.parametrize("n,c_in,P", [(64, 0, 2), (200, 1, 2), (200, 5, 3)])
def test_stats_bitwise_against_oracle(dev, n, c_in, P):
    x, called, y, cov, prep, S, Cs, trk = stats_case(n, c_in, P, seed=n + c_in)
    ref = R.stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"])
    got = dev.assoc_stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"])
    for name in ("beta", "se", "t", "p"):
        assert_bitwise(got[name], ref[name], name)
    assert np.isnan(ref["beta"][:4]).all() and np.isnan(ref["p"][:4]).all()          # monomorphic twice, N = 0, all het (a constant dosage: D = 0)
    assert np.isfinite(ref["beta"][4:, : P - 1]).all() and np.isfinite(ref["p"][4:, : P - 1]).all()
    assert np.isnan(ref["t"][4:, P - 1]).all() and (ref["se"][4:, P - 1] == 0.0).all()  # the constant phenotype
    assert (Cs != np.array(prep["total"])).any()                                        # missing calls reach the imputation term
    # any output may be NULL
    only = dev.assoc_stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"], outputs=("p",))
    assert_bitwise(only["p"], ref["p"], "p alone")


def test_stats_refusals(lib):
    from ferromic_amd import _abi

    rows, K = 2, 2
    S, trk = np.zeros(rows * K, np.int64), np.ones(rows, np.uint32)
    total, e, yy, out = np.zeros(K, np.int64), np.zeros(K, np.int32), np.ones(1), np.zeros(rows)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ptr(S), ptr(S), ptr(trk), ptr(trk), ptr(trk), rows, ptr(total), ptr(e), ptr(yy), 10, 1, 1, ptr(out), None, None, None]
    assert lib.fmh_assoc_stats(*good) == _abi.FMH_OK
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert lib.fmh_assoc_stats(*args) == _abi.FMH_ERR_INVALID, i
    for i, v in ((9, 3), (9, (1 << 22) + 1), (11, 0), (10, 64)):   # n - c - 2 = 0, n > 2^22, P == 0, c + P > 64
        args = list(good)
        args[i] = v
        assert lib.fmh_assoc_stats(*args) == _abi.FMH_ERR_INVALID, (i, v)
    args = list(good)
    args[5] = 0
    args[0] = None
    assert lib.fmh_assoc_stats(*args) == _abi.FMH_OK              # no rows: nothing is read


# ---- the definition against ordinary least squares --------------------------------------------------------------------------------------
def test_definition_against_least_squares(dev, capsys):
    worst_beta = worst_t = 0.0
    for n in (64, 200, 1000):
        for c_in in (0, 1, 5):
            rng = np.random.default_rng(1000 + n + c_in)
            rows = 12
            freq = rng.uniform(0.2, 0.8, size=(rows, 1))
            x = (rng.random((rows, 2 * n)) < freq).astype(np.uint8)
            called = np.repeat(rng.random((rows, n)) > 0.05, 2, axis=1)
            cov = rng.normal(size=(n, c_in)) * 3.0 + 1.0 if c_in else None
            c, g = R.genotypes(x, called)
            y = rng.normal(size=(n, 2)) + 10.0
            y[:, 0] += 0.8 * g[5]                                   # one planted effect
            if c_in:
                y += cov[:, :1] * 0.5
            prep = dev.assoc_prepare(y, cov)
            S, Cs = R.sums(x, called, prep.values)
            trk = R.tracks(x, called)
            got = dev.assoc_stats(S, Cs, *trk, prep.total, prep.exponent, prep.yy, n, prep.n_basis)
            for r in range(rows):
                mu = g[r].sum() / c[r].sum()
                dosage = np.where(c[r] == 1, g[r].astype(np.float64), mu)
                design = np.column_stack([dosage, np.ones(n)] + ([cov] if c_in else []))
                for p in range(2):
                    coef, _, rank, _ = np.linalg.lstsq(design, y[:, p], rcond=None)
                    assert rank == design.shape[1]
                    resid = y[:, p] - design @ coef
                    sigma2 = resid @ resid / (n - design.shape[1])
                    se = np.sqrt(sigma2 * np.linalg.inv(design.T @ design)[0, 0])
                    t = coef[0] / se
                    db, dt = abs(got["beta"][r, p] - coef[0]) / se, abs(got["t"][r, p] - t) / max(1.0, abs(t))
                    worst_beta, worst_t = max(worst_beta, db), max(worst_t, dt)
                    assert db <= 1e-6 and dt <= 1e-6, (n, c_in, r, p, db, dt)
            assert abs(got["t"][5, 0]) == np.abs(got["t"][:, 0]).max()   # the planted row stands out
    with capsys.disabled():
        print(f"\nassoc vs least squares: worst |beta - ols| / se = {worst_beta:.3e}, worst |t - ols| / max(1, |t|) = {worst_t:.3e}")


# ---- the p-value ------------------------------------------------------------------------------------------------------------------------
def library_p(dev, df, targets):
    """t and p as fmh_assoc_stats computes them, and the oracle's p of the same inputs, for rows built to land near the target |t|: no basis,
    e = 0, n = df + 2 samples all called with two hets, so D = 2 - 4 / n; one phenotype column per target with a = S = 2^20 (0 for t = 0)
    and yy = a^2 / D * (1 + df / t^2), which makes t^2 = a^2 df / (D rss) the target's."""
    n = df + 2
    D = 2.0 - 4.0 / n
    a = float(1 << 20)
    trk = (np.array([n - 2], np.uint32), np.array([2], np.uint32), np.array([0], np.uint32))
    t_out, p_out, p_ref = [], [], []
    for at in range(0, len(targets), 64):
        part = targets[at:at + 64]
        S = np.array([[0 if t == 0.0 else 1 << 20 for t in part]], dtype=np.int64)
        yy = np.array([1.0 if t == 0.0 else a * a / D * (1.0 + df / (t * t)) for t in part])
        zero = [0] * len(part)
        got = dev.assoc_stats(S, np.zeros_like(S), *trk, zero, zero, yy, n, 0)
        ref = R.stats(S, np.zeros_like(S), *trk, zero, zero, yy, n, 0)
        t_out.append(got["t"][0]), p_out.append(got["p"][0]), p_ref.append(ref["p"][0])
    return np.concatenate(t_out), np.concatenate(p_out), np.concatenate(p_ref)


def test_p_value_against_scipy(dev, capsys):
    """The LIBRARY's p over the whole grid: df in {1, 2, 10, 997}, |t| from 0 to 40 - both branches of the incomplete beta function, p down to
    1e-200 - bitwise equal to the oracle's loop and within relative 1e-9 of scipy at the t the library itself reports."""
    sps = pytest.importorskip("scipy.stats")
    worst = 0.0
    targets = [0.0, 1e-8, 1e-3] + np.linspace(0.05, 40.0, 400).tolist()
    for df in (1, 2, 10, 997):
        t, p, p_oracle = library_p(dev, df, targets)
        assert np.isfinite(t).all() and np.isfinite(p).all() and t[0] == 0.0 and p[0] == 1.0
        assert np.allclose(t, targets, rtol=1e-6, atol=0.0) and t.max() > 39.9, "the rows cover the grid"
        a, x = df / 2.0, df / (df + t * t)
        first = x < (a + 1.0) / (a + 2.5)
        assert first.sum() > 100 and (~first).sum() >= 3, "both branches are taken"
        assert R.same_f64(p, p_oracle), df
        ref = 2.0 * sps.t.sf(np.abs(t), df)
        rel = np.abs(p - ref) / ref
        worst = max(worst, float(rel.max()))
        assert (rel <= 1e-9).all(), (df, t[rel.argmax()], p[rel.argmax()], ref[rel.argmax()])
    with capsys.disabled():
        print(f"\nassoc p-value (fmh_assoc_stats) vs scipy: worst relative error {worst:.3e}")


def test_p_value_against_integration(dev):
    """No scipy involved: the library's p against Simpson integration of the density (forced), where the integral is well conditioned."""
    for df in (1, 2, 10, 50):
        t, p, _ = library_p(dev, df, [0.1, 0.5, 1.0, 2.0, 3.5])
        for ti, pi in zip(t, p):
            ref = R.student_t_two_sided(float(ti), df, integrate=True)
            assert abs(pi - ref) <= 1e-8 * ref, (df, ti, pi, ref)


# ---- ferromic.AssociationScan.from_sums -------------------------------------------------------------------------------------------------
def test_from_sums_round_trip():
    import ferromic as fm

    n, c_in, P = 200, 5, 3
    x, called, y, cov, prep, S, Cs, trk = stats_case(n, c_in, P, seed=77)
    ref = R.stats(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"])
    positions = np.arange(S.shape[0], dtype=np.int64) * 10 + 3
    kept = np.flatnonzero(~prep["dropped"])
    scan = fm.AssociationScan.from_sums(S, Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"], positions=positions,
                                        covariates_kept=kept, covariates_dropped=np.flatnonzero(prep["dropped"]))
    assert len(scan) == S.shape[0] and scan.df == n - prep["n_basis"] - 2
    for name in ("beta", "se", "t", "p"):
        assert_bitwise(getattr(scan, name), ref[name], name)
    N = trk[0].astype(np.int64) + trk[1] + trk[2]
    assert np.array_equal(scan.n_called, N.astype(np.uint32))
    with np.errstate(invalid="ignore", divide="ignore"):
        freq = (trk[1].astype(np.float64) + 2.0 * trk[2]) / (2.0 * N)
    assert R.same_f64(scan.alt_frequency, freq)
    assert np.array_equal(scan.positions, positions) and np.array_equal(scan.covariates_kept, kept)
    assert scan.covariates_dropped.size == 0
    assert "AssociationScan(samples=200, sites=40, phenotypes=3, covariates=5, df=193)" == repr(scan)
    with pytest.raises(ValueError):
        fm.AssociationScan.from_sums(S[:3], Cs, *trk, prep["total"], prep["exponent"], prep["yy"], n, prep["n_basis"])
