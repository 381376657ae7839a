"""Oracle of the f-statistics, written from the definition in include/ferromic_hip.h and sharing nothing with the kernel or the C code.

A cohort is an allele matrix x [rows][cols] (uint8) and a called matrix [rows][cols] (bool) or None = everything called; groups are G boolean
column masks [G][cols].  A row is, against all groups at once and in this order: multiallelic when a called member of any group carries an
allele above 1, incomplete when a member of any group is not called, else usable with a_g = members of g whose allele is 1.  The table is
summed in integers that cannot wrap (int64 where rows x n^2 stays below 2^62, Python ints otherwise); f4 and the jackknife are
fractions.Fraction."""

import math
from fractions import Fraction

import numpy as np


def moment_count(G):
    return 1 + G + G * (G + 1) // 2


def pair_slot(G, i, j):
    """Slot of sum a_i a_j: the upper triangle row-major, diagonal included, behind the count and the G linear sums."""
    i, j = min(i, j), max(i, j)
    return 1 + G + sum(G - k for k in range(i)) + (j - i)


def classify(x, called, masks):
    """(a [rows][G] int64, multiallelic [rows] bool, incomplete [rows] bool) of every row against all groups."""
    masks = np.asarray(masks, dtype=bool)
    union = masks.any(axis=0)
    everyone = np.ones(x.shape, dtype=bool) if called is None else called
    multi = ((x > 1) & everyone)[:, union].any(axis=1)
    incomplete = ~multi & (~everyone)[:, union].any(axis=1)
    ones = ((x == 1) & everyone).astype(np.int64)
    a = ones @ masks.T.astype(np.int64)
    return a, multi, incomplete


def moments(x, called, masks, blocks):
    """(table [n_blocks][M] uint64, multiallelic [n_blocks] uint64, incomplete [n_blocks] uint64)."""
    masks = np.asarray(masks, dtype=bool)
    G = masks.shape[0]
    a, multi, incomplete = classify(x, called, masks)
    usable = ~multi & ~incomplete
    largest = int(masks.sum(axis=1).max())
    table = np.zeros((len(blocks), moment_count(G)), dtype=np.uint64)
    n_multi = np.zeros(len(blocks), dtype=np.uint64)
    n_incomplete = np.zeros(len(blocks), dtype=np.uint64)
    for b, (begin, end) in enumerate(blocks):
        rows = slice(int(begin), int(end))
        ab = a[rows][usable[rows]]
        if ab.shape[0] * largest * largest >= 1 << 62:
            ab = ab.astype(object)  # Python ints
        products = ab.T @ ab
        out = [int(ab.shape[0])] + [int(v) for v in ab.sum(axis=0)] if ab.shape[0] else [0] * (1 + G)
        out += [int(products[i, j]) if ab.shape[0] else 0 for i in range(G) for j in range(i, G)]
        table[b] = np.array(out, dtype=np.uint64)
        n_multi[b] = multi[rows].sum()
        n_incomplete[b] = incomplete[rows].sum()
    return table, n_multi, n_incomplete


def f4(slice_, sizes, A, B, C, D, unbiased):
    """(exact value or None for NaN, |biased part|, sum of |h terms used|) as Fractions: the block's sum of the estimator of
    (p_A - p_B)(p_C - p_D)."""
    G = len(sizes)
    n = [int(s) for s in sizes]
    S = lambda i, j: int(slice_[pair_slot(G, i, j)])  # noqa: E731
    biased = (Fraction(S(A, C), n[A] * n[C]) - Fraction(S(A, D), n[A] * n[D]) - Fraction(S(B, C), n[B] * n[C]) + Fraction(S(B, D), n[B] * n[D]))
    total, h_abs, nan = biased, Fraction(0), False
    if unbiased:
        for x, y, sign in ((A, C, -1), (A, D, +1), (B, C, +1), (B, D, -1)):
            if x != y:
                continue
            if n[x] < 2:
                nan = True
                continue
            h = Fraction(n[x] * int(slice_[1 + x]) - S(x, x), n[x] * n[x] * (n[x] - 1))
            total += sign * h
            h_abs += abs(h)
    return (None if nan else total), abs(biased), h_abs


def jackknife(num, den, weight=None):
    """The weighted delete-one-block jackknife of sum(num) / sum(den) in exact fractions (the inputs are taken as the floats they are):
    dict(estimate, jackknife_estimate, var as Fractions or None for NaN, se, z as floats, blocks)."""
    num = [Fraction(float(v)) for v in num]
    den = [Fraction(float(v)) for v in den]
    w = den if weight is None else [Fraction(float(v)) for v in weight]
    keep = [j for j in range(len(num)) if w[j] != 0]
    g = len(keep)
    out = dict(estimate=None, jackknife_estimate=None, var=None, se=math.nan, z=math.nan, blocks=g)
    sum_num, sum_den, n = sum(num[j] for j in keep), sum(den[j] for j in keep), sum(w[j] for j in keep)
    if g == 0 or sum_den == 0:
        return out
    theta = sum_num / sum_den
    out["estimate"] = theta
    if g == 1:
        out["jackknife_estimate"] = theta
        return out
    drop = {j: (sum_num - num[j]) / (sum_den - den[j]) for j in keep}
    theta_j = g * theta - sum((1 - w[j] / n) * drop[j] for j in keep)
    var = Fraction(0)
    for j in keep:
        h = n / w[j]
        tau = h * theta - (h - 1) * drop[j]
        var += (tau - theta_j) ** 2 / (h - 1)
    var /= g
    out.update(jackknife_estimate=theta_j, var=var, se=sqrt_fraction(var))
    out["z"] = float(theta) / out["se"] if out["se"] != 0 else math.copysign(math.inf, float(theta)) if theta != 0 else math.nan
    return out


def sqrt_fraction(v):
    """sqrt of a non-negative Fraction to well within one ulp of f64: an integer square root of v scaled by 2^200."""
    if v == 0:
        return 0.0
    shift = 200
    scaled = (v.numerator << (2 * shift)) // v.denominator
    return float(Fraction(math.isqrt(scaled), 1 << shift))
