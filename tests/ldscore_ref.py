"""The LD-score oracle, written from the definition in include/ferromic_hip.h (LD scores and LD score regression): per ordered pair of rows the
six integers and r^2 of tests/clump_ref.py, the correction as one Python float expression, q by math.ldexp and Python's round (half to even),
Python-int sums; the regression as plain loops over Python floats.  No bit planes, no tiles, no symmetry, no partner ranges: it shares
nothing with the kernel or the host twin.  Also the checksum of ferromic_amd/csrc/ldscore_host_check.cpp."""

import math
import struct

import numpy as np

from tests import clump_ref as R

MASK64 = (1 << 64) - 1
ONE = 1 << 40


def term(c, adjust):
    """q of a pair's counts, or None when the pair is skipped."""
    r2 = R.r2_of(c)
    if math.isnan(r2):
        return None
    t = r2
    if adjust:
        n = int(c[0])
        if n < 3:
            return None
        t = r2 - (1.0 - r2) / float(n - 2)
    return round(math.ldexp(t, 40))


_pairs = {}


def pair_table(dosage):
    """counts of every unordered pair of rows of a dosage table, made once per table (keyed by its bytes)."""
    dosage = np.ascontiguousarray(dosage, dtype=np.uint8)
    key = (dosage.shape, dosage.tobytes())
    if key not in _pairs:
        K = dosage.shape[0]
        d = dosage.astype(np.int64)
        called = (d < R.NOT_CALLED).astype(np.int64)
        g = d * called
        # integer matrix products, exact in int64: the same six sums R.counts gives per pair (checked against it in the CPU test)
        table = np.stack([called @ called.T, g @ called.T, called @ g.T, (g * g) @ called.T, called @ (g * g).T, g @ g.T], axis=-1)
        _pairs[key] = table.reshape(K, K, 6)
    return _pairs[key]


def ld_scores(dosage, x, window, adjust, counts_of=None):
    """The definition over a dosage table [K][n] and positions x [K] (None: x = k).  Returns a dict: q int64 [K], partners, counted, scores
    float64 [K], and what the tests' conditions ask about: negative_terms.  The pair counts come from pair_table, or per pair from
    `counts_of` (clump_ref.counts) when one is given."""
    dosage = np.asarray(dosage, dtype=np.uint8)
    K = dosage.shape[0]
    xs = [int(v) for v in (np.arange(K) if x is None else x)]
    table = None if counts_of is not None else pair_table(dosage)
    q, partners, counted, negative = [0] * K, [0] * K, [0] * K, 0
    for i in range(K):
        for j in range(K):
            if abs(xs[j] - xs[i]) > window:
                continue
            partners[i] += 1
            c = counts_of(dosage[i], dosage[j]) if counts_of is not None else tuple(int(v) for v in table[i, j])
            v = term(c, adjust)
            if v is None:
                continue
            counted[i] += 1
            q[i] += v
            negative += v < 0
    scores = [math.nan if counted[k] == 0 else float(q[k]) * 2.0 ** -40 for k in range(K)]
    return dict(q=np.array(q, dtype=np.int64).reshape(K), partners=np.array(partners, dtype=np.uint32).reshape(K), counted=np.array(counted, dtype=np.uint32).reshape(K),
                scores=np.array(scores, dtype=np.float64).reshape(K), negative_terms=negative)


def values(q, counted):
    return np.array([math.nan if int(c) == 0 else float(int(v)) * 2.0 ** -40 for v, c in zip(q, counted)], dtype=np.float64).reshape(len(q))


# ---- the regression ----------------------------------------------------------------------------------------------------------------------------
def _solve(s, fixed, a):
    w, x, xx, y, xy = s
    if fixed:
        return a, (xy - a * x) / xx
    det = w * xx - x * x
    return (xx * y - x * xy) / det, (w * xy - x * y) / det


def _se(pseudo):
    B = len(pseudo)
    mean = 0.0
    for v in pseudo:
        mean += v
    mean /= float(B)
    ss = 0.0
    for v in pseudo:
        ss += (v - mean) * (v - mean)
    return math.sqrt(ss / float(B - 1) / float(B))


def regress(chi2, score, N, M, blocks=200, intercept=None, weights=None):
    """The definition's LD score regression; a dict of the outputs plus `w` and `x`, the last fit's weights and regressor over the used sites."""
    N, M = float(N), float(M)
    fixed = intercept is not None
    y, l, lw = [], [], []
    for k in range(len(chi2)):
        wk = float(score[k] if weights is None else weights[k])
        if not (math.isfinite(chi2[k]) and math.isfinite(score[k]) and math.isfinite(wk)):
            continue
        y.append(float(chi2[k]))
        l.append(float(score[k]))
        lw.append(wk)
    U = len(y)
    B = min(int(blocks), U)
    P = 1 if fixed else 2
    if not (math.isfinite(N) and math.isfinite(M) and N > 0 and M > 0) or blocks < 2 or B < 2 or U < 2 * P * B or any(v < 0 for v in y):
        raise ValueError("refused")
    sum_y = sum_l = 0.0
    for i in range(U):
        sum_y += y[i]
        sum_l += l[i]
    mean_y, mean_l = sum_y / float(U), sum_l / float(U)
    a = float(intercept) if fixed else 1.0
    h = M * (mean_y - 1.0) / (N * mean_l)
    x = [N * l[i] / M for i in range(U)]
    w = [0.0] * U

    def sums(lo, hi):
        s = [0.0] * 5
        for i in range(lo, hi):
            wx = w[i] * x[i]
            s[0] += w[i]
            s[1] += wx
            s[2] += wx * x[i]
            s[3] += w[i] * y[i]
            s[4] += wx * y[i]
        return s

    for _ in range(3):
        hc = 0.0 if h < 0.0 else 1.0 if h > 1.0 else h
        for i in range(U):
            c = a + ((hc * N) * max(l[i], 1.0)) / M
            w[i] = 1.0 / (max(lw[i], 1.0) * (2.0 * (c * c)))
        a, h = _solve(sums(0, U), fixed, a)
    block = [sums(b * U // B, (b + 1) * U // B) for b in range(B)]
    pseudo_a, pseudo_h = [], []
    for b in range(B):
        s = [0.0] * 5
        for o in range(B):
            if o != b:
                for z in range(5):
                    s[z] += block[o][z]
        ab, hb = _solve(s, fixed, a)
        pseudo_a.append(float(B) * a - float(B - 1) * ab)
        pseudo_h.append(float(B) * h - float(B - 1) * hb)
    srt = sorted(y)
    median = srt[U // 2] if U % 2 else (srt[U // 2 - 1] + srt[U // 2]) / 2.0
    return dict(h2=h, h2_se=_se(pseudo_h), intercept=a, intercept_se=math.nan if fixed else _se(pseudo_a), ratio=(a - 1.0) / (mean_y - 1.0), mean_chi2=mean_y,
                lambda_gc=median / 0.4549364231195724, n_used=U, blocks=B, w=w, x=x, y=y)


# ---- the stand-alone program's checksum ----------------------------------------------------------------------------------------------------------
def bits_of(v):
    return 0x7FF8000000000000 if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", v))[0]


def checksum(result):
    """What ldscore_host_check prints for the sums: (terms, hash)."""
    h = terms = 0
    for k in range(len(result["q"])):
        q, c, p = int(result["q"][k]) & MASK64, int(result["counted"][k]), int(result["partners"][k])
        h = (h + q * ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) + c * (2 * k + 1) + p * (4 * k + 3) + bits_of(float(result["scores"][k])) * (6 * k + 5)) & MASK64
        terms += c
    return terms, h
