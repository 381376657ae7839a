"""The relatedness oracle, written from the definition in include/ferromic_hip.h (fmh_kinship_counts, fmh_kinship_stats,
fmh_kinship_unrelated): per-genotype `called` and dosage from the u8 matrix plus the called mask, the four tables as int64 products of the
indicator matrices, the estimators in numpy float64 with the header's operation order, the greedy rule in plain Python."""

import numpy as np


def genotype_classes(x, called, samples=None, keep=None):
    """(c, H, R, A) as [n][kept rows] int64 0/1 matrices.  x: [rows][2 * samples] uint8 alleles; called: the same shape bool, or None;
    samples: sample numbers (None: all); keep: [rows] bool (None: all)."""
    rows, cols = x.shape
    a = x.reshape(rows, cols // 2, 2).astype(np.int64)
    ok = (a <= 1).all(axis=2)  # an allele above 1 un-calls that genotype only
    if called is not None:
        ok &= called.reshape(rows, cols // 2, 2).all(axis=2)
    g = a.sum(axis=2)
    if keep is not None:
        k = np.asarray(keep, dtype=bool)
        ok, g = ok[k], g[k]
    if samples is not None:
        s = np.asarray(samples, dtype=np.int64)
        ok, g = ok[:, s], g[:, s]
    c = ok.astype(np.int64).T
    return c, ((g == 1) & ok).astype(np.int64).T, ((g == 0) & ok).astype(np.int64).T, ((g == 2) & ok).astype(np.int64).T


def tables(x, called, samples=None, keep=None):
    """(both, het_het, ibs0, het_hom) as [n][n] uint64."""
    c, H, R, A = genotype_classes(x, called, samples, keep)
    V = R + A
    out = (c @ c.T, H @ H.T, R @ A.T + A @ R.T, H @ V.T)
    return tuple(t.astype(np.uint64) for t in out)


def tables_brute(x, called, samples=None, keep=None):
    """The same by three nested loops over (i, j, row), from the definition's words."""
    rows, cols = x.shape
    samples = list(range(cols // 2)) if samples is None else [int(s) for s in samples]
    kept = [r for r in range(rows) if keep is None or keep[r]]
    n = len(samples)
    both, het_het, ibs0, het_hom = (np.zeros((n, n), dtype=np.uint64) for _ in range(4))

    def genotype(r, s):
        for col in (2 * s, 2 * s + 1):
            if (called is not None and not called[r, col]) or x[r, col] > 1:
                return None
        return int(x[r, 2 * s]) + int(x[r, 2 * s + 1])

    for i, si in enumerate(samples):
        for j, sj in enumerate(samples):
            for r in kept:
                gi, gj = genotype(r, si), genotype(r, sj)
                if gi is None or gj is None:
                    continue
                both[i, j] += 1
                het_het[i, j] += gi == 1 and gj == 1
                ibs0[i, j] += (gi == 0 and gj == 2) or (gi == 2 and gj == 0)
                het_hom[i, j] += gi == 1 and gj != 1
    return both, het_het, ibs0, het_hom


def stats(both, het_het, ibs0, het_hom):
    """(kinship, ibs_distance) as float64 with the header's operation order."""
    both, het_het, ibs0, het_hom = (np.asarray(t, dtype=np.uint64) for t in (both, het_het, ibs0, het_hom))
    het_i = het_het + het_hom
    het_j = het_het + het_hom.T
    m = np.minimum(het_i, het_j)
    hom = het_hom + het_hom.T
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.float64(0.5) - (hom + np.uint64(4) * ibs0).astype(np.float64) / (np.uint64(4) * m).astype(np.float64)
        dist = (hom + np.uint64(2) * ibs0).astype(np.float64) / (np.uint64(2) * both).astype(np.float64)
    phi[m == 0] = np.nan
    dist[both == 0] = np.nan
    return phi, dist


def unrelated(phi, threshold):
    """The greedy rule: until no remaining pair exceeds the threshold, remove the remaining sample with the most remaining partners
    (phi[i][j] > threshold, NaN never), the highest index on a tie."""
    n = len(phi)
    keep = [True] * n
    while True:
        counts = [sum(1 for j in range(n) if j != i and keep[j] and phi[i][j] > threshold) if keep[i] else 0 for i in range(n)]
        most = max(counts, default=0)
        if most == 0:
            return np.array(keep, dtype=bool)
        keep[max(i for i in range(n) if counts[i] == most)] = False
