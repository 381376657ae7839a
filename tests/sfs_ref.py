"""Numpy oracle of the site frequency spectra, written from the definition in include/ferromic_hip.h and sharing nothing with the kernel.

A cohort is an allele matrix x [rows][cols] (uint8) and a called matrix [rows][cols] (bool) or None = everything called; a group is a
boolean column mask with n members.  Against a group a row is, in this order: multiallelic when a called member carries an allele above 1,
incomplete when a member is not called, else binned at k = members whose allele is 1.  The statistics are plain Python floats."""

import math

import numpy as np


def classify(x, called, mask):
    """(k [rows] int64, multiallelic [rows] bool, incomplete [rows] bool) of every row against one group."""
    mask = np.asarray(mask, dtype=bool)
    xs = x[:, mask]
    cs = np.ones(xs.shape, dtype=bool) if called is None else called[:, mask]
    multi = ((xs > 1) & cs).any(axis=1)
    incomplete = ~multi & (~cs).any(axis=1)
    k = ((xs == 1) & cs).sum(axis=1).astype(np.int64)
    return k, multi, incomplete


def sfs(x, called, mask, windows):
    """1-D spectra: (counts [n_windows][n + 1] uint64, multiallelic [n_windows], incomplete [n_windows])."""
    n = int(np.asarray(mask, dtype=bool).sum())
    k, multi, incomplete = classify(x, called, mask)
    usable = ~multi & ~incomplete
    counts = np.zeros((len(windows), n + 1), dtype=np.uint64)
    n_multi = np.zeros(len(windows), dtype=np.uint64)
    n_incomplete = np.zeros(len(windows), dtype=np.uint64)
    for w, (begin, end) in enumerate(windows):
        rows = slice(int(begin), int(end))
        counts[w] = np.bincount(k[rows][usable[rows]], minlength=n + 1)
        n_multi[w] = multi[rows].sum()
        n_incomplete[w] = incomplete[rows].sum()
    return counts, n_multi, n_incomplete


def sfs_joint(x, called, mask0, mask1, row_begin, row_count):
    """Joint spectrum: (counts [n0 + 1][n1 + 1] uint64, multiallelic, incomplete)."""
    n0, n1 = int(np.asarray(mask0, dtype=bool).sum()), int(np.asarray(mask1, dtype=bool).sum())
    rows = slice(row_begin, row_begin + row_count)
    k0, m0, i0 = classify(x[rows], None if called is None else called[rows], mask0)
    k1, m1, i1 = classify(x[rows], None if called is None else called[rows], mask1)
    multi = m0 | m1
    incomplete = ~multi & (i0 | i1)
    usable = ~multi & ~incomplete
    flat = np.bincount(k0[usable] * (n1 + 1) + k1[usable], minlength=(n0 + 1) * (n1 + 1))
    return flat.astype(np.uint64).reshape(n0 + 1, n1 + 1), int(multi.sum()), int(incomplete.sum())


def folded(counts):
    counts = [int(c) for c in counts]
    n = len(counts) - 1
    return [counts[j] if j == n - j else counts[j] + counts[n - j] for j in range(n // 2 + 1)]


def stats(counts):
    """The statistics of one spectrum of n + 1 bins as a dict of Python ints and floats (NaN rules as in the header)."""
    counts = [int(c) for c in counts]
    n = len(counts) - 1
    nan = float("nan")
    out = dict(sites=sum(counts), segregating_sites=sum(counts[1:n]), pi_sum=nan, theta_w_sum=nan, theta_h_sum=nan, tajima_d=nan, fay_wu_h=nan)
    if n < 2:
        return out
    S = out["segregating_sites"]
    pairs = n * (n - 1)
    pi = math.fsum(counts[k] * 2 * k * (n - k) / pairs for k in range(n + 1))
    theta_h = math.fsum(counts[k] * 2 * k * k / pairs for k in range(1, n))
    a1 = math.fsum(1.0 / i for i in range(1, n))
    a2 = math.fsum(1.0 / (i * i) for i in range(1, n))
    out.update(pi_sum=pi, theta_w_sum=S / a1, theta_h_sum=theta_h, fay_wu_h=pi - theta_h)
    if S == 0 or n < 4:
        return out
    b1 = (n + 1) / (3 * (n - 1))
    b2 = 2 * (n * n + n + 3) / (9 * n * (n - 1))
    c1 = b1 - 1 / a1
    c2 = b2 - (n + 2) / (a1 * n) + a2 / (a1 * a1)
    e1 = c1 / a1
    e2 = c2 / (a1 * a1 + a2)
    out["tajima_d_sd"] = math.sqrt(e1 * S + e2 * S * (S - 1))
    out["tajima_d"] = (pi - S / a1) / out["tajima_d_sd"]
    return out
