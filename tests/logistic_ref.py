"""The logistic association scan's oracle, written from the definitions in include/ferromic_hip.h (fmh_assoc_homalt_sums,
fmh_logistic_null, fmh_logistic_score, fmh_logistic_stats) and sharing no code with the library.  homalt_sums() is numpy int64 arithmetic on
the genotype classes; null_model(), score() and stats() are plain sequential loops over Python floats (IEEE f64, no fused multiply-add), so
the library's integers and doubles can be compared bit for bit.  exp, log and erfc are the C library's, called through ctypes, as the
definition names them; dense_reference() is the INDEPENDENT evaluation (numpy Newton fit and linear solves on the unquantised floats) that
the accuracy test measures the definition against."""

import ctypes
import ctypes.util
import math

import numpy as np

from tests import assoc_ref as A

MAX_SAMPLES = 1 << 21
MAX_COLUMNS = 64
MAX_STEPS = 25
TOLERANCE = 1e-8
FITTED, ONE_CLASS, NOT_CONVERGED, PIVOT, ZERO_WEIGHT, BASIS_LOST = range(6)

same_f64 = A.same_f64


def _libm(name):
    try:
        lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
        return fn
    except (OSError, AttributeError):
        return getattr(math, name)


_exp, _log, _erfc = _libm("exp"), _libm("log"), _libm("erfc")


# ---- H: numpy over the genotype classes ---------------------------------------------------------------------------------------------------
def homalt_sums(x, called, values, samples=None):
    """H = (c [g == 2]) @ V, [rows][K] int64."""
    c, g = A.genotypes(x, called, samples)
    v = np.asarray(values, dtype=np.int64)
    assert v.shape[0] == c.shape[1] and np.abs(v).max(initial=0) <= A.MAX_VALUE
    return ((g == 2) & (c == 1)).astype(np.int64) @ v


# ---- the null model: plain loops over Python floats ---------------------------------------------------------------------------------------
def _covariate_basis(cov):
    """fmh_assoc_prepare's steps 1 and 2."""
    basis, dropped = [], []
    for j in range(cov.shape[1]):
        x = A._centre([float(v) for v in cov[:, j]])
        r0 = math.sqrt(A._seq_dot(x, x))
        x = A._project_off(x, basis)
        r = math.sqrt(A._seq_dot(x, x))
        drop = r0 == 0.0 or r <= r0 * 2.0 ** -26
        dropped.append(drop)
        if not drop:
            basis.append([v / r for v in x])
    return basis, dropped


def _weights(X, beta):
    """mu, w per sample, or None at the first w that is not > 0."""
    n, d = len(X[0]), len(X)
    mu, w = [0.0] * n, [0.0] * n
    for i in range(n):
        eta = 0.0
        for j in range(d):
            eta += X[j][i] * beta[j]
        mu[i] = 1.0 / (1.0 + _exp(-eta))
        w[i] = mu[i] * (1.0 - mu[i])
        if not w[i] > 0.0:
            return None
    return mu, w


def _fit(X, y, n_cases):
    """Returns (reason, steps, mu, w)."""
    n, d = len(y), len(X)
    if n_cases == 0 or n_cases == n:
        return ONE_CLASS, 0, None, None
    beta = [0.0] * d
    beta[0] = _log(float(n_cases) / float(n - n_cases)) / X[0][0]
    steps = 0
    for step in range(1, MAX_STEPS + 1):
        got = _weights(X, beta)
        if got is None:
            return ZERO_WEIGHT, steps, None, None
        mu, w = got
        grad = [0.0] * d
        Am = [[0.0] * d for _ in range(d)]
        for j in range(d):
            g = 0.0
            for i in range(n):
                g += X[j][i] * (y[i] - mu[i])
            grad[j] = g
            for k in range(j + 1):
                a = 0.0
                for i in range(n):
                    a += (X[j][i] * w[i]) * X[k][i]
                Am[j][k] = a
        L = [[0.0] * d for _ in range(d)]
        for j in range(d):
            for k in range(j + 1):
                s = Am[j][k]
                for m in range(k):
                    s = s - L[j][m] * L[k][m]
                if k == j:
                    if not s > 0.0:
                        return PIVOT, steps, None, None
                    L[j][j] = math.sqrt(s)
                else:
                    L[j][k] = s / L[k][k]
        z = [0.0] * d
        for j in range(d):
            s = grad[j]
            for m in range(j):
                s = s - L[j][m] * z[m]
            z[j] = s / L[j][j]
        delta = [0.0] * d
        for j in range(d - 1, -1, -1):
            s = z[j]
            for m in range(j + 1, d):
                s = s - L[m][j] * delta[m]
            delta[j] = s / L[j][j]
        worst, finite = 0.0, True
        for j in range(d):
            beta[j] = beta[j] + delta[j]
            a = abs(delta[j])
            if not math.isfinite(a):
                finite = False
            if a > worst:
                worst = a
        steps = step
        if finite and worst < TOLERANCE:
            got = _weights(X, beta)
            if got is None:
                return ZERO_WEIGHT, steps, None, None
            return FITTED, steps, got[0], got[1]
    return NOT_CONVERGED, steps, None, None


def null_model(phenotypes, covariates=None):
    """Returns dict(values: list per batch of [n][Pb * W] int32, exponent [P][W], total [P][W] (Python ints), fitted, reason, iterations,
    n_cases [P], n_basis, dropped [c_in] bool, batch)."""
    y = np.asarray(phenotypes, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    n, P = y.shape
    assert 1 <= n <= MAX_SAMPLES and P >= 1 and np.isin(y, (0.0, 1.0)).all()
    cov = np.zeros((n, 0)) if covariates is None else np.asarray(covariates, dtype=np.float64)
    basis, dropped = _covariate_basis(cov)
    c = len(basis)
    W = c + 3
    assert W <= MAX_COLUMNS and n >= W
    X = [[1.0 / math.sqrt(float(n))] * n] + basis
    d = c + 1
    columns, exponent, total, fitted, reason, iterations, n_cases = [], [], [], [], [], [], []
    for p in range(P):
        yp = [float(v) for v in y[:, p]]
        cases = sum(1 for v in yp if v == 1.0)
        why, steps, mu, w = _fit(X, yp, cases)
        u = []
        if why == FITTED:
            for j in range(d):
                z = [math.sqrt(w[i]) * X[j][i] for i in range(n)]
                r0 = math.sqrt(A._seq_dot(z, z))
                z = A._project_off(z, u)
                r = math.sqrt(A._seq_dot(z, z))
                if r0 == 0.0 or r <= r0 * 2.0 ** -26:
                    why = BASIS_LOST
                    break
                u.append([v / r for v in z])
        cols, es = [], []
        if why == FITTED:
            real = [[math.sqrt(w[i]) * u[j][i] for i in range(n)] for j in range(d)] + [[yp[i] - mu[i] for i in range(n)], list(w)]
            for col in real:
                v, e = A._quantise(col)
                cols.append(v)
                es.append(e)
        else:
            cols, es = [[0] * n for _ in range(W)], [0] * W
        columns.append(cols)
        exponent.append(es)
        total.append([sum(col) for col in cols])
        fitted.append(why == FITTED)
        reason.append(why)
        iterations.append(steps)
        n_cases.append(cases)
    batch = MAX_COLUMNS // W
    values = []
    for first in range(0, P, batch):
        part = [col for cols in columns[first:first + batch] for col in cols]
        values.append(np.array(part, dtype=np.int64).T.astype(np.int32).reshape(n, len(part)))
    return dict(values=values, exponent=np.array(exponent, dtype=np.int32), total=total, fitted=np.array(fitted, dtype=bool),
                reason=np.array(reason, dtype=np.int32), iterations=np.array(iterations, dtype=np.int32), n_cases=np.array(n_cases, dtype=np.uint64),
                n_basis=c, dropped=np.array(dropped, dtype=bool), batch=batch)


# ---- score, variance and statistics -----------------------------------------------------------------------------------------------------
def score(S, C, H, hom_ref, het, hom_alt, total, exponent, c):
    """One phenotype batch: S, C [rows][Pb * W], H [rows][Pb], total and exponent flat [Pb * W].  Returns (U, Vr) [rows][Pb]."""
    rows = len(hom_ref)
    W = c + 3
    total = [int(t) for t in np.asarray(total, dtype=object).reshape(-1)]
    exponent = [int(e) for e in np.asarray(exponent).reshape(-1)]
    Pb = len(total) // W
    U, V = np.full((rows, Pb), np.nan), np.full((rows, Pb), np.nan)
    for r in range(rows):
        h, alt = int(het[r]), int(hom_alt[r])
        N = int(hom_ref[r]) + h + alt
        n_alt = h + 2 * alt
        if N == 0 or n_alt == 0 or n_alt == 2 * N:
            continue
        mu = float(n_alt) / float(N)

        def a_of(k):
            return math.ldexp(float(int(S[r][k])) + mu * float(total[k] - int(C[r][k])), -exponent[k])

        for p in range(Pb):
            o = p * W
            kw = o + c + 2
            U[r, p] = a_of(o + c + 1)
            vr = math.ldexp(float(int(S[r][kw]) + 2 * int(H[r][p])) + (mu * mu) * float(total[kw] - int(C[r][kw])), -exponent[kw])
            for j in range(c + 1):
                a = a_of(o + j)
                vr = vr - a * a
            V[r, p] = vr
    return U, V


def stats(U, V):
    """chi2, z, p, beta, se, shaped as U."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    out = {k: np.full(U.shape, np.nan) for k in ("chi2", "z", "p", "beta", "se")}
    for idx in np.ndindex(U.shape):
        u, v = float(U[idx]), float(V[idx])
        if not v > 0.0 or u != u:
            continue
        chi2 = u * u / v
        out["chi2"][idx] = chi2
        out["z"][idx] = u / math.sqrt(v)
        out["p"][idx] = _erfc(math.sqrt(chi2 / 2.0))
        out["beta"][idx] = u / v
        out["se"][idx] = 1.0 / math.sqrt(v)
    return out


def scan(x, called, phenotypes, covariates=None, samples=None):
    """The whole pipeline from numpy's integer sums: dict of the seven [rows][P] tables plus the null model under "model"."""
    model = null_model(phenotypes, covariates)
    c, W, batch = model["n_basis"], model["n_basis"] + 3, model["batch"]
    trk = A.tracks(x, called, samples)
    P = len(model["fitted"])
    U, V = np.zeros((len(trk[0]), P)), np.zeros((len(trk[0]), P))
    for b, values in enumerate(model["values"]):
        first = b * batch
        Pb = values.shape[1] // W
        S, Cs = A.sums(x, called, values, samples)
        H = homalt_sums(x, called, values[:, c + 2::W], samples)
        tot = [t for row in model["total"][first:first + Pb] for t in row]
        U[:, first:first + Pb], V[:, first:first + Pb] = score(S, Cs, H, *trk, tot, model["exponent"][first:first + Pb].reshape(-1), c)
    out = dict(score=U, variance=V, **stats(U, V))
    for p in np.flatnonzero(~model["fitted"]):
        for table in out.values():
            table[:, p] = np.nan
    out["model"] = model
    out["tracks"] = trk
    return out


# ---- the independent reference: dense algebra on the unquantised floats ----------------------------------------------------------------------
def dense_reference(dosage, y, covariates=None):
    """dosage [n] (mean-imputed already), y [n] 0/1, covariates [n][c] or None.  A numpy Newton fit of the null model run to a gradient
    below 1e-12, then U = g'(y - mu) and V = g'Wg - g'WX (X'WX)^-1 X'Wg by numpy.linalg.solve."""
    n = y.shape[0]
    X = np.ones((n, 1)) if covariates is None or covariates.shape[1] == 0 else np.column_stack([np.ones(n), covariates])
    beta = np.zeros(X.shape[1])
    for _ in range(200):
        mu = 1.0 / (1.0 + np.exp(-(X @ beta)))
        grad = X.T @ (y - mu)
        if np.abs(grad).max() < 1e-12:
            break
        beta = beta + np.linalg.solve(X.T @ (X * (mu * (1.0 - mu))[:, None]), grad)
    else:
        raise AssertionError("the reference fit did not converge")
    w = mu * (1.0 - mu)
    U = dosage @ (y - mu)
    xwg = X.T @ (w * dosage)
    V = dosage @ (w * dosage) - xwg @ np.linalg.solve(X.T @ (X * w[:, None]), xwg)
    return float(U), float(V)
