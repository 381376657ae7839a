"""The genotype QC oracle, written from the definition in include/ferromic_hip.h (fmh_genotype_counts, fmh_hwe_exact,
fmh_genotype_site_stats, fmh_genotype_site_weights, fmh_genotype_sample_stats): `called` and dosage per genotype from the u8 matrix plus
the called mask in numpy, the row and column sums, the Hardy-Weinberg exact test as a loop over plain Python floats (and as exact
fractions.Fraction enumeration), the estimators in numpy float64 with the header's operation order."""

import math
from fractions import Fraction

import numpy as np

HWE_MAX_GENOTYPES = 1 << 26
FIXED_ONE = 2147483648.0  # 2^31: the weights' fixed point


def classes(x, called, samples=None):
    """(c, g): [rows][n] bool `called` and int64 dosage of the selected samples.  x: [rows][2 * samples] uint8; called: the same shape
    bool, or None; samples: sample numbers (None: all)."""
    rows, cols = x.shape
    a = x.reshape(rows, cols // 2, 2).astype(np.int64)
    c = (a <= 1).all(axis=2)  # an allele above 1 un-calls that genotype only
    if called is not None:
        c &= called.reshape(rows, cols // 2, 2).all(axis=2)
    g = a.sum(axis=2)
    if samples is not None:
        s = np.asarray(samples, dtype=np.int64)
        c, g = c[:, s], g[:, s]
    return c, g


def site_tracks(x, called, samples=None):
    """hom_ref, het, hom_alt as [rows] uint32: the keep mask does not apply."""
    c, g = classes(x, called, samples)
    return tuple((c & (g == k)).sum(axis=1).astype(np.uint32) for k in (0, 1, 2))


def sample_tables(x, called, samples=None, keep=None):
    """hom_ref, het, hom_alt as [n] uint64 over the kept rows."""
    c, g = classes(x, called, samples)
    if keep is not None:
        k = np.asarray(keep, dtype=bool)
        c, g = c[k], g[k]
    return tuple((c & (g == k)).sum(axis=0).astype(np.uint64) for k in (0, 1, 2))


def weighted_called(x, called, weights, samples=None, keep=None):
    """[n] uint64: the sum over the kept rows of w_r c_s(r) (u64 arithmetic: exact below 2^32 rows)."""
    c, _ = classes(x, called, samples)
    w = np.asarray(weights, dtype=np.uint64)
    if keep is not None:
        k = np.asarray(keep, dtype=bool)
        c, w = c[k], w[k]
    return (c.astype(np.uint64) * w[:, None]).sum(axis=0, dtype=np.uint64)


def counts_brute(x, called, samples=None, keep=None, weights=None):
    """(site tracks, sample tables, weighted) by nested loops over (row, sample), from the definition's words."""
    rows, cols = x.shape
    samples = list(range(cols // 2)) if samples is None else [int(s) for s in samples]
    site = np.zeros((3, rows), dtype=np.uint32)
    sample = np.zeros((3, len(samples)), dtype=np.uint64)
    weighted = [0] * len(samples)
    for r in range(rows):
        for i, s in enumerate(samples):
            genotype = 0
            for col in (2 * s, 2 * s + 1):
                if genotype is None or (called is not None and not called[r, col]) or x[r, col] > 1:
                    genotype = None
                else:
                    genotype += int(x[r, col])
            if genotype is None:
                continue
            site[genotype, r] += 1
            if keep is None or keep[r]:
                sample[genotype, i] += 1
                if weights is not None:
                    weighted[i] += int(weights[r])
    return tuple(site), tuple(sample), np.array(weighted, dtype=np.uint64)


# ---- the Hardy-Weinberg exact test ------------------------------------------------------------------------------------------------------
def _walk(N, rare, mid, visit):
    """The header's walk: visit(x, t) at mid, then down, then up; a walk stops once t == 0.0."""
    visit(mid, 1.0)
    t, x, r = 1.0, mid, (rare - mid) // 2
    c = N - x - r
    while x >= 2:
        t = (t * float(x * (x - 1))) / float(4 * (r + 1) * (c + 1))
        x, r, c = x - 2, r + 1, c + 1
        if t == 0.0:
            break
        visit(x, t)
    t, x, r = 1.0, mid, (rare - mid) // 2
    c = N - x - r
    while x + 2 <= rare:
        t = (t * float(4 * r * c)) / float((x + 2) * (x + 1))
        x, r, c = x + 2, r - 1, c - 1
        if t == 0.0:
            break
        visit(x, t)


def hwe_p(hom_ref, het, hom_alt):
    """One site, plain Python floats (IEEE doubles), the operation order of the header."""
    hom_ref, het, hom_alt = int(hom_ref), int(het), int(hom_alt)
    N = hom_ref + het + hom_alt
    if N == 0 or N > HWE_MAX_GENOTYPES:
        return math.nan
    rare = 2 * min(hom_ref, hom_alt) + het
    common = 2 * N - rare
    if rare == 0:
        return 1.0
    mid = rare * common // (2 * N)
    if (mid ^ rare) & 1:
        mid += 1
    state = {"S": 0.0, "t_obs": 0.0, "P": 0.0}

    def first(x, t):
        state["S"] += t
        if x == het:
            state["t_obs"] = t

    def second(x, t):
        if t <= state["t_obs"]:
            state["P"] += t

    _walk(N, rare, mid, first)
    _walk(N, rare, mid, second)
    p = state["P"] / state["S"]
    return 1.0 if p > 1.0 else p


def hwe(hom_ref, het, hom_alt):
    return np.array([hwe_p(a, b, c) for a, b, c in zip(hom_ref, het, hom_alt)], dtype=np.float64)


def hwe_exact_fraction(hom_ref, het, hom_alt):
    """The exact p as a Fraction: every het count of the site's parity, weights as exact rationals relative to x = rare's parity floor."""
    N = hom_ref + het + hom_alt
    rare = 2 * min(hom_ref, hom_alt) + het
    if rare == 0:
        return Fraction(1)
    x = rare & 1
    r = (rare - x) // 2
    c = N - x - r
    w = Fraction(1)
    weights = {x: w}
    while x + 2 <= rare:
        w = w * (4 * r * c) / ((x + 2) * (x + 1))
        x, r, c = x + 2, r - 1, c - 1
        weights[x] = w
    obs = weights[het]
    return sum(v for v in weights.values() if v <= obs) / sum(weights.values())


# ---- estimators ---------------------------------------------------------------------------------------------------------------------------
def site_stats(hom_ref, het, hom_alt, n_samples):
    hom_ref, het, hom_alt = (np.asarray(a, dtype=np.uint64) for a in (hom_ref, het, hom_alt))
    N = hom_ref + het + hom_alt
    n_alt = np.uint64(2) * hom_alt + het
    n_ref = np.uint64(2) * N - n_alt
    two_n_1 = np.where(N > 0, np.uint64(2) * N - np.uint64(1), np.uint64(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        call_rate = N.astype(np.float64) / np.float64(n_samples) if n_samples else np.full(N.shape, np.nan)
        p = n_alt.astype(np.float64) / (np.uint64(2) * N).astype(np.float64)
        maf = np.minimum(p, np.float64(1.0) - p)
        f_is = np.float64(1.0) - (het * two_n_1).astype(np.float64) / (n_alt * n_ref).astype(np.float64)
        expected = (n_alt * n_ref).astype(np.float64) / two_n_1.astype(np.float64)
    p[N == 0] = np.nan
    maf[N == 0] = np.nan
    f_is[n_alt * n_ref == 0] = np.nan
    expected[N == 0] = np.nan
    return dict(call_rate=call_rate, alt_frequency=p, maf=maf, f_is=f_is, expected_het=expected)


def site_weights(hom_ref, het, hom_alt):
    hom_ref, het, hom_alt = (np.asarray(a, dtype=np.uint64) for a in (hom_ref, het, hom_alt))
    N = hom_ref + het + hom_alt
    n_alt = np.uint64(2) * hom_alt + het
    n_ref = np.uint64(2) * N - n_alt
    den = np.where(N > 0, N * (np.uint64(2) * N - np.uint64(1)), np.uint64(1))
    e = np.where(N > 0, (n_alt * n_ref).astype(np.float64) / den.astype(np.float64), 0.0)
    return np.rint(e * FIXED_ONE).astype(np.uint32)


def sample_stats(hom_ref, het, hom_alt, kept_rows, weighted=None):
    hom_ref, het, hom_alt = (np.asarray(a, dtype=np.uint64) for a in (hom_ref, het, hom_alt))
    called = hom_ref + het + hom_alt
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(call_rate=called.astype(np.float64) / np.float64(kept_rows) if kept_rows else np.full(called.shape, np.nan),
                   het_rate=het.astype(np.float64) / called.astype(np.float64))
        out["het_rate"][called == 0] = np.nan
        if weighted is not None:
            weighted = np.asarray(weighted, dtype=np.uint64)
            f = np.float64(1.0) - het.astype(np.float64) / (weighted.astype(np.float64) / np.float64(FIXED_ONE))
            f[weighted == 0] = np.nan
            out["f"] = f
    return out
