"""The polygenic score's oracle, written from the definitions in include/ferromic_hip.h (fmh_score_sums, fmh_score_exponents,
fmh_score_values, fmh_score_stats) and sharing no code with the library.  sums() is numpy int64 arithmetic on the genotype table;
exponents(), values() and stats() are plain loops over Python floats and ints (IEEE f64, no fused multiply-add, arbitrary-precision
integers), so the library's integers and doubles can be compared bit for bit."""

import math

import numpy as np

MAX_VALUE = 1 << 30
MAX_ROWS = 1 << 21
MAX_COLUMNS = 64
MODES = ("mean", "center", "zero")


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


def sums(x, called, values, called_values=None, samples=None):
    """S = (c g)^T @ V and C = c^T @ U, [n][K] int64, exact while rows <= 2^21 and |V|, |U| <= 2^30.  C is None without U."""
    c, g = genotypes(x, called, samples)
    v = np.asarray(values, dtype=np.int64)
    assert v.shape[0] == c.shape[0] and np.abs(v).max(initial=0) <= MAX_VALUE and c.shape[0] <= MAX_ROWS
    if called_values is None:
        return g.T @ v, None
    u = np.asarray(called_values, dtype=np.int64)
    assert u.shape == v.shape and np.abs(u).max(initial=0) <= MAX_VALUE
    return g.T @ v, c.T @ u


def tracks(x, called, samples=None):
    """hom_ref, het, hom_alt per row, uint32."""
    c, g = genotypes(x, called, samples)
    return tuple(((g == k) & (c == 1)).sum(axis=1).astype(np.uint32) for k in (0, 1, 2))


def sample_classes(x, called, samples=None, keep=None):
    """hom_ref, het, hom_alt per sample over the kept rows, uint64."""
    c, g = genotypes(x, called, samples)
    if keep is not None:
        c, g = c[np.asarray(keep, dtype=bool)], g[np.asarray(keep, dtype=bool)]
    return tuple(((g == k) & (c == 1)).sum(axis=0).astype(np.uint64) for k in (0, 1, 2))


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


def digit_planes(values):
    """digits() of a whole array: [4] + values.shape int64."""
    v = np.asarray(values, dtype=np.int64).copy()
    out = []
    for _ in range(4):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) >> 8
    assert not v.any()
    return np.stack(out)


def item_accumulators(x, called, values, item_rows):
    """What the digit accumulators of the work items hold at the end: [row block][digit][n][K] int64 (every sample, no list)."""
    _, g = genotypes(x, called)
    d = digit_planes(values)   # [4][rows][K]
    out = []
    for first in range(0, g.shape[0], item_rows):
        block = slice(first, first + item_rows)
        out.append(np.stack([g[block].T @ d[j, block] for j in range(4)]))
    return np.stack(out)


# ---- the host functions: plain loops over Python floats and ints ---------------------------------------------------------------------------
def _weights(weights):
    w = np.asarray(weights, dtype=np.float64)
    return w.reshape(-1, 1) if w.ndim == 1 else w


def exponents(weights):
    """e_k = the largest integer with 2 max_r |w_rk| 2^e_k <= 2^30: max = f 2^x, f in [0.5, 1): 30 - x when f == 0.5, else 29 - x; 0 for zeros."""
    w = _weights(weights)
    out = []
    for k in range(w.shape[1]):
        mx = 0.0
        for v in w[:, k]:
            v = float(v)
            assert math.isfinite(v)
            mx = max(mx, abs(v))
        if mx == 0.0:
            out.append(0)
            continue
        f, x = math.frexp(mx)
        out.append(30 - x if f == 0.5 else 29 - x)
    return out


def _rint(v):
    return int(round(v))   # round() is round-half-even, as rint


def values(weights, e, hom_ref=None, het=None, hom_alt=None):
    """Returns dict(V [rows][K], U [rows][K] or None, total [K] Python ints or None, used [rows] bool)."""
    w = _weights(weights)
    rows, K = w.shape
    with_tracks = hom_ref is not None
    V, U, used = [], [], []
    total = [0] * K
    for r in range(rows):
        wr = [float(v) for v in w[r]]
        N, n_alt = 1, 0
        if with_tracks:
            N = int(hom_ref[r]) + int(het[r]) + int(hom_alt[r])
            n_alt = int(het[r]) + 2 * int(hom_alt[r])
        use = N != 0 and any(v != 0.0 for v in wr)
        used.append(use)
        if not use:
            V.append([0] * K)
            U.append([0] * K)
            continue
        V.append([_rint(math.ldexp(wr[k], e[k])) for k in range(K)])
        if with_tracks:
            mu = float(n_alt) / float(N)
            U.append([_rint(math.ldexp(mu * wr[k], e[k])) for k in range(K)])
            for k in range(K):
                total[k] += U[-1][k]
    assert all(abs(v) <= MAX_VALUE for row in V + (U if with_tracks else []) for v in row)
    return dict(V=np.array(V, dtype=np.int32).reshape(rows, K), U=np.array(U, dtype=np.int32).reshape(rows, K) if with_tracks else None,
                total=total if with_tracks else None, used=np.array(used, dtype=bool))


def stats(S, C, total, e, mode):
    """f64 [n][K]: ldexp of the exact integer, formed in Python ints."""
    S = np.asarray(S)
    n, K = S.shape
    out = np.zeros((n, K), dtype=np.float64)
    for i in range(n):
        for k in range(K):
            x = int(S[i][k])
            if mode == "mean":
                x += int(total[k]) - int(C[i][k])
            elif mode == "center":
                x -= int(C[i][k])
            else:
                assert mode == "zero"
            assert abs(x) < 1 << 53
            out[i][k] = math.ldexp(float(x), -int(e[k]))
    return out


def score(x, called, weights, samples=None, mode="mean"):
    """The whole definition end to end: dict(score, S, C, total, e, used, rows_used, n_called, dosage_sum)."""
    w = _weights(weights)
    e = exponents(w)
    trk = tracks(x, called, samples)
    val = values(w, e, *trk)
    S, C = sums(x, called, val["V"], val["U"], samples)
    keep = (w != 0.0).any(axis=1)
    ref, het, alt = sample_classes(x, called, samples, keep)
    return dict(score=stats(S, C, val["total"], e, mode), S=S, C=C, total=val["total"], e=e, used=val["used"], rows_used=int(val["used"].sum()),
                n_called=ref + het + alt, dosage_sum=het + np.uint64(2) * alt)


def same_f64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
