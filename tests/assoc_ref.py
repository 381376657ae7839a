"""The association scan's oracle, written from the definitions in include/ferromic_hip.h (fmh_assoc_sums, fmh_assoc_prepare,
fmh_assoc_stats) and sharing no code with the library.  sums() is numpy int64 arithmetic on the genotype table; prepare() and stats() are
plain sequential loops over Python floats (IEEE f64, no fused multiply-add), so the library's integers and doubles can be compared bit for
bit; student_t_two_sided() is an INDEPENDENT evaluation of the tail (scipy where it imports, numerical integration otherwise) for the
accuracy test of the library's continued fraction."""

import ctypes
import ctypes.util
import math

import numpy as np

MAX_VALUE = 1 << 30
MAX_SAMPLES = 1 << 22
MAX_COLUMNS = 64


def genotypes(x, called, samples=None):
    """x, called: [rows][2 n] allele values and called flags (None: every entry is called).  Returns (c, g): [rows][n] called flags and
    dosages of the selected samples."""
    x = np.asarray(x).astype(np.int64)
    ok = (np.ones(x.shape, dtype=bool) if called is None else np.asarray(called).astype(bool)) & (x <= 1)
    c = ok[:, 0::2] & ok[:, 1::2]
    g = (x[:, 0::2] + x[:, 1::2]) * c
    if samples is not None:
        idx = np.asarray(samples, dtype=np.int64)
        c, g = c[:, idx], g[:, idx]
    return c.astype(np.int64), g.astype(np.int64)


def sums(x, called, values, samples=None):
    """S = (c g) @ V and C = c @ V, [rows][K] int64, exact while n <= 2^22 and |V| <= 2^30."""
    c, g = genotypes(x, called, samples)
    v = np.asarray(values, dtype=np.int64)
    assert v.shape[0] == c.shape[1] and np.abs(v).max(initial=0) <= MAX_VALUE
    return g @ v, c @ v


def tracks(x, called, samples=None):
    """hom_ref, het, hom_alt per row, uint32."""
    c, g = genotypes(x, called, samples)
    return tuple(((g == k) & (c == 1)).sum(axis=1).astype(np.uint32) for k in (0, 1, 2))


def digits(v):
    """The signed base-256 digits d0 .. d3 of an integer |v| <= 2^30: v = sum d_j 256^j, d_j in [-128, 127]."""
    v = int(v)
    out = []
    for _ in range(4):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) >> 8
    assert v == 0
    return out


# ---- prepare: plain loops over Python floats -----------------------------------------------------------------------------------------
def _seq_dot(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s += u * v
    return s


def _centre(x):
    s = 0.0
    for v in x:
        s += v
    mean = s / float(len(x))
    return [v - mean for v in x]


def _project_off(x, basis):
    for _ in range(2):
        for q in basis:
            d = _seq_dot(q, x)
            x = [v - d * w for v, w in zip(x, q)]
    return x


def _exponent(x):
    mx = 0.0
    for v in x:
        mx = max(mx, abs(v))
    if mx == 0.0:
        return 0
    f, ex = math.frexp(mx)
    return 31 - ex if f == 0.5 else 30 - ex


def _quantise(x):
    e = _exponent(x)
    v = [int(round(math.ldexp(u, e))) for u in x]   # round() is round-half-even, as rint
    assert all(abs(u) <= MAX_VALUE for u in v)
    return v, e


def prepare(phenotypes, covariates=None):
    """Returns dict(values [n][K] int32, exponent [K], total [K] (Python ints), yy [P], n_basis, dropped [c_in] bool)."""
    y = np.asarray(phenotypes, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    n, P = y.shape
    cov = np.zeros((n, 0)) if covariates is None else np.asarray(covariates, dtype=np.float64)
    basis, dropped = [], []
    for j in range(cov.shape[1]):
        x = _centre([float(v) for v in cov[:, j]])
        r0 = math.sqrt(_seq_dot(x, x))
        x = _project_off(x, basis)
        r = math.sqrt(_seq_dot(x, x))
        drop = r0 == 0.0 or r <= r0 * 2.0 ** -26
        dropped.append(drop)
        if not drop:
            basis.append([v / r for v in x])
    c = len(basis)
    assert n - c - 2 >= 1 and c + P <= MAX_COLUMNS
    columns, exponent, yy = [], [], []
    for q in basis:
        v, e = _quantise(q)
        columns.append(v)
        exponent.append(e)
    for p in range(P):
        x = _project_off(_centre([float(v) for v in y[:, p]]), basis)
        v, e = _quantise(x)
        columns.append(v)
        exponent.append(e)
        s = 0.0
        for u in v:
            w = math.ldexp(float(u), -e)
            s += w * w
        yy.append(s)
    values = np.array(columns, dtype=np.int64).T.astype(np.int32).reshape(n, c + P)
    return dict(values=values, exponent=np.array(exponent, dtype=np.int32), total=[sum(col) for col in columns], yy=np.array(yy, dtype=np.float64),
                n_basis=c, dropped=np.array(dropped, dtype=bool))


# ---- stats ---------------------------------------------------------------------------------------------------------------------------
def _libm_lgamma():
    """The C library's lgamma, which the definition names (CPython's math.lgamma is an implementation of its own)."""
    try:
        lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        fn = lib.lgamma
        fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
        return fn
    except (OSError, AttributeError):
        return math.lgamma


_lgamma = _libm_lgamma()


def _beta_cf(a, b, x):
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 10001):
        dm = float(m)
        m2 = 2.0 * dm
        aa = dm * (b - dm) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h = h * (d * c)
        aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h = h * delta
        if abs(delta - 1.0) < 1e-15:
            break
    return h


def t_tail_definition(t, df):
    """The header's p: I_x(df/2, 1/2) by the modified Lentz continued fraction."""
    t2 = t * t
    if t2 == 0.0:
        return 1.0
    x = df / (df + t2)
    if x == 0.0:
        return 0.0
    xc = t2 / (df + t2)
    a, b = df / 2.0, 0.5
    front = math.exp(_lgamma(a + b) - _lgamma(a) - _lgamma(b) + a * math.log(x) + b * math.log(xc))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _beta_cf(a, b, x) / a
    return 1.0 - front * _beta_cf(b, a, xc) / b


def stats(S, C, hom_ref, het, hom_alt, total, exponent, yy, n, c):
    """beta, se, t, p [rows][P] float64 by the header's formulas, one Python float operation per arithmetic step."""
    rows, P = len(hom_ref), len(yy)
    out = {k: np.full((rows, P), np.nan) for k in ("beta", "se", "t", "p")}
    df = n - c - 2
    for r in range(rows):
        h, alt = int(het[r]), int(hom_alt[r])
        N = int(hom_ref[r]) + h + alt
        if N == 0:
            continue
        n_alt = h + 2 * alt
        mu = float(n_alt) / float(N)

        def a_of(k):
            return math.ldexp(float(int(S[r][k])) + mu * float(int(total[k]) - int(C[r][k])), -int(exponent[k]))

        D = float(h + 4 * alt) - float(n_alt * n_alt) / float(N)
        for k in range(c):
            a = a_of(k)
            D = D - a * a
        if not D > 0.0:
            continue
        for p in range(P):
            a = a_of(c + p)
            beta = a / D
            rss = float(yy[p]) - a * a / D
            if rss < 0.0:
                rss = 0.0
            se = math.sqrt(rss / float(df) / D)
            out["beta"][r, p], out["se"][r, p] = beta, se
            if se == 0.0:
                continue
            t = beta / se
            out["t"][r, p], out["p"][r, p] = t, t_tail_definition(t, float(df))
    return out


def student_t_two_sided(t, df, integrate=False):
    """Independent of the library's algorithm: scipy's survival function where scipy imports, else (or with `integrate`) Simpson integration
    of the density in u = atan(t / sqrt(df)) (the tail is the integral of cos^(df-1) u over [u, pi/2], normalised)."""
    if not integrate:
        try:
            from scipy import stats as sps

            return float(2.0 * sps.t.sf(abs(t), df))
        except ImportError:
            pass
    u0 = math.atan(abs(t) / math.sqrt(df))
    steps = 20000

    def integral(lo, hi):
        hstep = (hi - lo) / steps
        s = math.cos(lo) ** (df - 1) + math.cos(hi) ** (df - 1)
        for i in range(1, steps):
            s += (4 if i % 2 else 2) * math.cos(lo + i * hstep) ** (df - 1)
        return s * hstep / 3.0

    return integral(u0, math.pi / 2) / integral(0.0, math.pi / 2)


def same_f64(a, b):
    """Bitwise equality of two float64 arrays, NaN positions equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))
