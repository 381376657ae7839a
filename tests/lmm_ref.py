"""Oracle of the mixed-model association scan, written from the definition in include/ferromic_hip.h (mixed-model association scan).  Nothing
here touches the device or the library under test.

projections(): T, quad and lin in np.longdouble from a genotype code table (tests/grm_ref.py: 0 hom-ref, 1 het, 2 hom-alt, 3 not called), with
the absolute sums the error bounds need.  null_fit() and stats(): the header's operation order as plain loops over Python floats (IEEE f64, no
fused multiply-add; math.log and math.pow are the C library's), on tests/assoc_ref.py's covariate basis.  dense(): a reference that shares no
algebra with either - no rotation, V = A + delta I and np.linalg.solve on the original floats."""

from __future__ import annotations

import math

import numpy as np

from tests import assoc_ref
from tests import grm_ref

U53 = 2.0 ** -53
MASK64 = (1 << 64) - 1
GRID_POINTS, GOLDEN_STEPS = 101, 40


# ---- projections ---------------------------------------------------------------------------------------------------------------------------------
def counts(code):
    return grm_ref.counts(code)


def mu_of(c, a):
    c, a = np.asarray(c, dtype=np.float64), np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c == 0, 0.0, a / np.where(c == 0, 1.0, c))


def dosages(code, swap_hom=False, missing_as_zero=False):
    """x [rows][n] float64: the dosage where called, else the row's mu (the exact f64 quotient a / c)."""
    c, a = counts(code)
    mu = mu_of(c, a)
    g = code.astype(np.float64)
    if swap_hom:
        g = np.where(code == 0, 2.0, np.where(code == 2, 0.0, g))
    return np.where(code <= 2, g, 0.0 if missing_as_zero else mu[:, None])


def projections(code, basis, weights, linear, swap_hom=False, missing_as_zero=False, transpose=False, weights_on_t=False):
    """dict(quad [rows][P], lin [rows][L] as float64 roundings of the longdouble sums, quad_bound, lin_bound: the derived bounds (not yet
    doubled), c, a).  The keyword arguments are what a wrong kernel would compute."""
    ld = np.longdouble
    B = np.asarray(basis, dtype=np.float64)
    if transpose:
        B = B.T
    W, Lm = np.asarray(weights, dtype=np.float64), np.asarray(linear, dtype=np.float64)
    x = dosages(code, swap_hom, missing_as_zero)
    n, K = B.shape
    T = x.astype(ld) @ B.astype(ld)                         # [rows][K]
    absT = np.abs(x).astype(ld) @ np.abs(B).astype(ld)      # sum_i |basis_ik x_i|
    E = (n + 2) * U53 * absT
    T2 = T if weights_on_t else T * T
    quad = T2 @ W.astype(ld).T
    lin = T @ Lm.astype(ld).T
    aW, aL = np.abs(W).astype(ld).T, np.abs(Lm).astype(ld).T
    lin_bound = E @ aL + (K + 2) * U53 * (np.abs(T) @ aL)
    quad_bound = (2 * np.abs(T) * E + E * E) @ aW + (K + 3) * U53 * ((T * T) @ aW)
    c, a = counts(code)
    return dict(quad=quad.astype(np.float64), lin=lin.astype(np.float64), quad_bound=quad_bound.astype(np.float64), lin_bound=lin_bound.astype(np.float64),
                c=c, a=a, T=T)


def worst_ratio(got, want, bound):
    """max |got - want| / (2 bound), an entry with a zero bound must be exact."""
    err, lim = np.abs(np.asarray(got, dtype=np.float64) - want), 2.0 * bound
    if err.size == 0:
        return 0.0
    assert np.all(err[lim == 0] == 0)
    return float((err / np.where(lim > 0, lim, 1.0)).max())


# ---- the null fit: plain loops ------------------------------------------------------------------------------------------------------------------
def covariate_basis(cov, n):
    """(Q as a list of columns, dropped flags): fmh_assoc_prepare's rule, as tests/assoc_ref.py states it."""
    basis, dropped = [], []
    for j in range(0 if cov is None else cov.shape[1]):
        x = assoc_ref._centre([float(v) for v in cov[:, j]])
        r0 = math.sqrt(assoc_ref._seq_dot(x, x))
        x = assoc_ref._project_off(x, basis)
        r = math.sqrt(assoc_ref._seq_dot(x, x))
        drop = r0 == 0.0 or r <= r0 * 2.0 ** -26
        dropped.append(drop)
        if not drop:
            basis.append([v / r for v in x])
    return basis, dropped


def _cholesky(a, q):
    for j in range(q):
        d = a[j][j]
        for k in range(j):
            d -= a[j][k] * a[j][k]
        if not d > 0.0:
            return False
        l = math.sqrt(d)
        a[j][j] = l
        for i in range(j + 1, q):
            s = a[i][j]
            for k in range(j):
                s -= a[i][k] * a[j][k]
            a[i][j] = s / l
    return True


def _cholesky_solve(l, q, b):
    b = list(b)
    for i in range(q):
        s = b[i]
        for k in range(i):
            s -= l[i][k] * b[k]
        b[i] = s / l[i][i]
    for i in range(q - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, q):
            s -= l[k][i] * b[k]
        b[i] = s / l[i][i]
    return b


def log_likelihood(lam, xr, yr, delta):
    """(l, dict(w, chol, xwy, b, R)) at delta; l = -inf where XWX is not positive definite or R is not positive."""
    n, q = len(lam), len(xr[0])
    w, log_v = [], 0.0
    for k in range(n):
        s = lam[k] + delta
        w.append(1.0 / s)
        log_v += math.log(s)
    xwx = [[0.0] * q for _ in range(q)]
    xwy = [0.0] * q
    for a in range(q):
        for b in range(a + 1):
            s = 0.0
            for k in range(n):
                s += w[k] * xr[k][a] * xr[k][b]
            xwx[a][b] = xwx[b][a] = s
        s = 0.0
        for k in range(n):
            s += w[k] * xr[k][a] * yr[k]
        xwy[a] = s
    ev = dict(w=w, chol=xwx, xwy=xwy, b=None, R=float("nan"))
    if not _cholesky(xwx, q):
        return -math.inf, ev
    log_det = 0.0
    for a in range(q):
        log_det += math.log(xwx[a][a])
    log_det = 2.0 * log_det
    b = _cholesky_solve(xwx, q, xwy)
    R = 0.0
    for k in range(n):
        fit = 0.0
        for a in range(q):
            fit += xr[k][a] * b[a]
        res = yr[k] - fit
        R += w[k] * (res * res)
    ev["b"], ev["R"] = b, R
    if not R > 0.0:
        return -math.inf, ev
    dof = float(n - q)
    return -0.5 * (dof * math.log(2.0 * 3.14159265358979323846 * R / dof) + log_v + log_det + dof), ev


def grid_point(i):
    return -5.0 + 0.1 * float(i)


def search(lam, xr, yr):
    """(log10 delta of the best point evaluated, l at the 101 grid points)."""
    f = lambda x: log_likelihood(lam, xr, yr, math.pow(10.0, x))[0]
    grid = [f(grid_point(i)) for i in range(GRID_POINTS)]
    best_x, best_ll = grid_point(0), grid[0]
    for i in range(1, GRID_POINTS):
        if grid[i] > best_ll:
            best_x, best_ll = grid_point(i), grid[i]
    gr = (math.sqrt(5.0) - 1.0) / 2.0
    lo, hi = max(best_x - 0.1, -5.0), min(best_x + 0.1, 5.0)
    c, d = hi - gr * (hi - lo), lo + gr * (hi - lo)
    fc, fd = f(c), f(d)
    if fc > best_ll:
        best_x, best_ll = c, fc
    if fd > best_ll:
        best_x, best_ll = d, fd
    for _ in range(GOLDEN_STEPS):
        if fc > fd:
            hi, d, fd = d, c, fc
            c = hi - gr * (hi - lo)
            fc = f(c)
            if fc > best_ll:
                best_x, best_ll = c, fc
        else:
            lo, c, fc = c, d, fd
            d = lo + gr * (hi - lo)
            fd = f(d)
            if fd > best_ll:
                best_x, best_ll = d, fd
    return best_x, grid


def null_fit(lam, U, Y, cov=None, fixed_delta=None):
    """The header's fmh_lmm_null.  Returns dict(q, dropped, delta, sigma_g2, sigma_e2, heritability, log_likelihood, at_boundary, reason, weights
    [P][n], linear [P (q + 1)][n], M [P][q][q], v [P][q], R [P], grid [P][101], log10_delta)."""
    lam = [max(float(v), 0.0) for v in np.asarray(lam, dtype=np.float64)]
    U = np.asarray(U, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)
    n, P = Y.shape
    cov = None if cov is None else np.asarray(cov, dtype=np.float64).reshape(n, -1)
    basis, dropped = covariate_basis(cov, n)
    c = len(basis)
    q = c + 1
    assert n - q - 1 >= 1 and P <= 16 and P * (q + 1) <= 64
    ones = 1.0 / math.sqrt(float(n))
    X = [[ones] + [basis[j][i] for j in range(c)] for i in range(n)]
    Ul = U.tolist()
    xr = [[assoc_ref._seq_dot([Ul[i][k] for i in range(n)], [X[i][j] for i in range(n)]) for j in range(q)] for k in range(n)]
    nan = float("nan")
    out = dict(q=q, dropped=np.array(dropped, dtype=bool), weights=np.zeros((P, n)), linear=np.zeros((P * (q + 1), n)), M=np.full((P, q, q), nan),
               v=np.full((P, q), nan), grid=np.full((P, GRID_POINTS), nan))
    for name in ("delta", "sigma_g2", "sigma_e2", "heritability", "log_likelihood", "R", "log10_delta"):
        out[name] = np.full(P, nan)
    out["at_boundary"], out["reason"] = np.zeros(P, dtype=bool), np.zeros(P, dtype=np.uint8)
    for p in range(P):
        y = [float(v) for v in Y[:, p]]
        r0 = math.sqrt(assoc_ref._seq_dot(y, y))
        res = assoc_ref._project_off(assoc_ref._centre(y), basis)
        r1 = math.sqrt(assoc_ref._seq_dot(res, res))
        if r0 == 0.0 or r1 <= r0 * 2.0 ** -26:
            out["reason"][p] = 1
            continue
        yr = [assoc_ref._seq_dot([Ul[i][k] for i in range(n)], y) for k in range(n)]
        if fixed_delta is None:
            x, grid = search(lam, xr, yr)
            out["grid"][p] = grid
            delta = math.pow(10.0, x)
            out["log10_delta"][p] = x
            out["at_boundary"][p] = x == -5.0 or x == 5.0
        else:
            delta = float(np.asarray(fixed_delta, dtype=np.float64).reshape(-1)[p])
            out["log10_delta"][p] = math.log10(delta)
        ll, ev = log_likelihood(lam, xr, yr, delta)
        w, R = ev["w"], ev["R"]
        out["delta"][p], out["sigma_g2"][p], out["log_likelihood"][p], out["R"][p] = delta, R / float(n - q), ll, R
        out["sigma_e2"][p], out["heritability"][p] = delta * (R / float(n - q)), 1.0 / (1.0 + delta)
        out["weights"][p] = w
        for j in range(q):
            out["linear"][p * (q + 1) + j] = [w[k] * xr[k][j] for k in range(n)]
        out["linear"][p * (q + 1) + q] = [w[k] * yr[k] for k in range(n)]
        M = [[0.0] * q for _ in range(q)]
        for j in range(q):
            col = _cholesky_solve(ev["chol"], q, [1.0 if i == j else 0.0 for i in range(q)])
            for i in range(q):
                M[i][j] = col[i]
        out["M"][p] = M
        out["v"][p] = [assoc_ref._seq_dot(M[i], ev["xwy"]) for i in range(q)]
    return out


# ---- statistics: plain loops --------------------------------------------------------------------------------------------------------------------
def stats(quad, lin, called, allele_count, M, v, R, n, tail=True):
    """beta, se, t, p [rows][P] by the header's formulas, one Python float operation per arithmetic step."""
    quad, lin = np.asarray(quad, dtype=np.float64), np.asarray(lin, dtype=np.float64)
    rows, P = quad.shape
    q = np.asarray(v).shape[1]
    df = n - q - 1
    out = {k: np.full((rows, P), np.nan) for k in ("beta", "se", "t", "p")}
    Ml, vl = np.asarray(M, dtype=np.float64).tolist(), np.asarray(v, dtype=np.float64).tolist()
    for r in range(rows):
        c, a = int(called[r]), int(allele_count[r])
        if c == 0 or a == 0 or a == 2 * c:
            continue
        for p in range(P):
            av = [float(x) for x in lin[r, p * (q + 1) : (p + 1) * (q + 1)]]
            aMa = 0.0
            for i in range(q):
                aMa += assoc_ref._seq_dot(Ml[p][i], av[:q]) * av[i]
            av_v = 0.0
            for i in range(q):
                av_v += av[i] * vl[p][i]
            D = float(quad[r, p]) - aMa
            num = av[q] - av_v
            if not D > 0.0:
                continue
            beta = num / D
            rss = float(R[p]) - num * num / D
            if rss < 0.0:
                rss = 0.0
            se = math.sqrt(rss / float(df) / D)
            out["beta"][r, p], out["se"][r, p] = beta, se
            if se == 0.0:
                continue
            t = beta / se
            out["t"][r, p] = t
            if tail:
                out["p"][r, p] = assoc_ref.t_tail_definition(t, float(df))
    return out


# ---- the dense reference: no rotation ---------------------------------------------------------------------------------------------------------------
def dense(code, A, delta, y, cov_kept=None):
    """beta, se, t [rows] of one phenotype by generalised least squares on the original floats: V = A + delta I,
    X1 = [1, kept covariates, mean-imputed dosage], beta = (X1^T V^-1 X1)^-1 X1^T V^-1 y, se from rss / df.  NaN on rows that are not
    polymorphic among the called."""
    code = np.asarray(code)
    rows, n = code.shape
    x = dosages(code)
    c, a = counts(code)
    V = np.asarray(A, dtype=np.float64) + float(delta) * np.eye(n)
    cols = [np.ones(n)] + ([] if cov_kept is None else [np.asarray(cov_kept, dtype=np.float64)[:, j] for j in range(np.asarray(cov_kept).shape[1])])
    X0 = np.stack(cols, axis=1)
    k = X0.shape[1] + 1
    df = n - k
    Vi_X0, Vi_y = np.linalg.solve(V, X0), np.linalg.solve(V, np.asarray(y, dtype=np.float64))
    out = {name: np.full(rows, np.nan) for name in ("beta", "se", "t")}
    for r in range(rows):
        if c[r] == 0 or a[r] == 0 or a[r] == 2 * c[r]:
            continue
        X1 = np.concatenate([X0, x[r][:, None]], axis=1)
        Vi_X1 = np.concatenate([Vi_X0, np.linalg.solve(V, x[r])[:, None]], axis=1)
        G = X1.T @ Vi_X1
        b = np.linalg.solve(G, X1.T @ Vi_y)
        res = np.asarray(y, dtype=np.float64) - X1 @ b
        rss = float(res @ np.linalg.solve(V, res))
        se = math.sqrt(rss / df * float(np.linalg.inv(G)[-1, -1]))
        out["beta"][r], out["se"][r], out["t"][r] = b[-1], se, b[-1] / se
    return out


# ---- a cohort with relatives: duplicated and half-sib-like samples ---------------------------------------------------------------------------------
def related_codes(rows, n, seed, missing=0.05):
    """[rows][n] codes: a third of the samples unrelated founders, then exact duplicates of founders and 'half sibs' that copy one haplotype
    of a founder and draw the other; `missing` of the genotypes not called; rows 0 .. 2: all hom-ref, all not called, all hom-alt."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.95, size=(rows, 1))
    founders = max(n // 3, 2)
    h0 = (rng.random((rows, n)) < freq).astype(np.uint8)
    h1 = (rng.random((rows, n)) < freq).astype(np.uint8)
    for s in range(founders, n):
        parent = int(rng.integers(0, founders))
        if s % 2 == 0:
            h0[:, s], h1[:, s] = h0[:, parent], h1[:, parent]  # a duplicate
        else:
            h0[:, s] = h0[:, parent]                             # shares one haplotype
    code = (h0 + h1).astype(np.uint8)
    code[rng.random((rows, n)) < missing] = 3
    if rows > 3:
        code[0], code[1], code[2] = 0, 3, 2
    return code


def grm_of(code):
    """A (standardized, denominator sites) by tests/grm_ref.py."""
    S, _, _, _, _, _, m = grm_ref.products(code, "standardized")
    return S / float(m)


# ---- the seeded case of ferromic_amd/csrc/lmm_host_check.cpp, and its two lines -------------------------------------------------------------------
def _unit(r):
    return float(r.next() >> 11) * 2.0 ** -53 - 0.5


def check_case(seed, rows, n, flat):
    r = grm_ref.SplitMix64(seed)
    d = np.zeros((rows, n), dtype=np.uint8)
    for k in range(rows):
        t, gaps = r.next() % 17, r.next() % 32
        for s in range(n):
            g = int(r.next() % 16 < t) + int(r.next() % 16 < t)
            if gaps == 0 or (gaps < 4 and r.next() % 4 == 0):
                g = 3
            d[k, s] = g
    h, hh = [], 0.0
    for _ in range(n):
        h.append(_unit(r))
        hh += h[-1] * h[-1]
    U = np.array([[(1.0 if i == k else 0.0) - 2.0 * h[i] * h[k] / hh for k in range(n)] for i in range(n)])
    lam = np.array([0.0 if r.next() % 4 == 0 else 4.0 * (_unit(r) + 0.5) for _ in range(n)])
    Y, cov = np.zeros((n, 2)), np.zeros((n, 3))
    for i in range(n):
        Y[i, 0] = 3.0 + _unit(r)
        Y[i, 1] = 1.5 if flat else _unit(r)
        cov[i, 0] = _unit(r)
        cov[i, 1] = 10.0 * _unit(r)
        cov[i, 2] = cov[i, 0]
    return d, U, lam, Y, cov


def twin(code, basis, weights, linear):
    """fmh_lmm_projections_host as plain loops over Python floats: (quad, lin) bit for bit."""
    code = np.asarray(code)
    rows, n = code.shape
    B, W, Lm = (np.asarray(a, dtype=np.float64).tolist() for a in (basis, weights, linear))
    K = len(B[0])
    x_all = dosages(code).tolist()
    quad, lin = np.zeros((rows, len(W))), np.zeros((rows, len(Lm)))
    for r in range(rows):
        x = x_all[r]
        T = [0.0] * K
        for i in range(n):
            xi, bi = x[i], B[i]
            for k in range(K):
                T[k] += bi[k] * xi
        for p, w in enumerate(W):
            s = 0.0
            for k in range(K):
                s += w[k] * (T[k] * T[k])
            quad[r, p] = s
        for j, l in enumerate(Lm):
            s = 0.0
            for k in range(K):
                s += l[k] * T[k]
            lin[r, j] = s
    return quad, lin


def bits_of(v) -> int:
    return grm_ref.bits_of(v)


def check_lines(seed, rows, n, flat):
    """(the checksum line, the searched deltas) lmm_host_check prints for this case."""
    d, U, lam, Y, cov = check_case(seed, rows, n, flat)
    searched = null_fit(lam, U, Y, cov)
    flags = int(searched["at_boundary"][0]) + 2 * int(searched["at_boundary"][1]) + 4 * int(searched["reason"][0]) + 8 * int(searched["reason"][1])
    fit = null_fit(lam, U, Y, cov, fixed_delta=[0.5, 2.0])
    q, P = fit["q"], 2
    quad, lin = twin(d, U, fit["weights"], fit["linear"])
    c, a = counts(d)
    st = stats(quad, lin, c, a, fit["M"], fit["v"], fit["R"], n)
    h = q * 1000003 + int(fit["dropped"][0]) + 2 * int(fit["dropped"][1]) + 4 * int(fit["dropped"][2])

    def add(values, offset):
        nonlocal h
        for e, v in enumerate(np.asarray(values, dtype=np.float64).reshape(-1)):
            h = (h + bits_of(v) * (2 * e + offset)) & MASK64

    add(fit["weights"], 1)
    add(fit["linear"], 3)
    add(fit["M"], 5)
    add(fit["v"], 7)
    add(fit["R"], 9)
    for e in range(rows):
        h = (h + int(c[e]) * ((0x9E3779B97F4A7C15 + e) & MASK64) + int(a[e]) * ((0xBF58476D1CE4E5B9 + e) & MASK64)) & MASK64
    for e in range(rows * P):
        h += bits_of(quad.reshape(-1)[e]) * (2 * e + 11) + bits_of(st["beta"].reshape(-1)[e]) * (2 * e + 13)
        h += bits_of(st["se"].reshape(-1)[e]) * (2 * e + 15) + bits_of(st["t"].reshape(-1)[e]) * (2 * e + 17)
        h &= MASK64
    add(lin, 19)
    finite = int(np.isfinite(st["p"]).sum())
    line = "lmm_host_check: %d rows x %d samples, q %d, %d finite, flags %d, checksum %016x" % (rows, n, q, finite, flags, h)
    return line, searched["delta"]
