"""numpy oracle of the genomic relationship matrix, written from the definition in include/ferromic_hip.h (genomic relationship matrix and
genotype PCA).  Nothing here touches the device or the library under test.

Genotype codes: 0 hom-ref, 1 het, 2 hom-alt, 3 not called (an entry uncalled, or an allele above 1).  Every f64 of values() is formed in
the header's operation order, so the library's host functions must reproduce the bits; the scale is a sequential sum (np.cumsum), not
numpy's pairwise one."""

from __future__ import annotations

import numpy as np

EPS = 2.0 ** -53
MASK64 = (1 << 64) - 1
METHODS = ("standardized", "centered")


def codes(x, called=None, samples=None, keep=None) -> np.ndarray:
    """[K][n] uint8 genotype codes of the kept rows of alleles x [rows][2 * samples] (called: bool of the same shape, or None)."""
    x = np.asarray(x)
    rows, cols = x.shape
    ok = np.ones((rows, cols), dtype=bool) if called is None else np.asarray(called, dtype=bool)
    ok = ok & (x <= 1)
    both = ok[:, 0::2] & ok[:, 1::2]
    g = x[:, 0::2].astype(np.uint8) + x[:, 1::2].astype(np.uint8)
    code = np.where(both, g, 3).astype(np.uint8)
    if samples is not None:
        code = code[:, np.asarray(samples, dtype=np.int64)]
    if keep is not None:
        code = code[np.asarray(keep, dtype=bool)]
    return np.ascontiguousarray(code)


def counts(code):
    """(c, a) uint32 per row: called genotypes and the sum of their dosages."""
    called = code <= 2
    return called.sum(axis=1).astype(np.uint32), np.where(called, code, 0).sum(axis=1).astype(np.uint32)


def values(c, a, method="standardized"):
    """(usable bool [K], p [K] (NaN where c = 0), z [K][3] (zero on rows that are not usable), scale, n_usable) in the stated order."""
    assert method in METHODS
    c64, a64 = np.asarray(c, dtype=np.int64), np.asarray(a, dtype=np.int64)
    usable = (c64 >= 1) & (a64 > 0) & (a64 < 2 * c64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(c64 == 0, np.nan, a64.astype(np.float64) / (2 * c64).astype(np.float64))
    z = np.zeros((c64.size, 3), dtype=np.float64)
    pu = p[usable]
    mean = 2.0 * pu
    var = mean * (1.0 - pu)
    zu = np.stack([0.0 - mean, 1.0 - mean, 2.0 - mean], axis=1)
    if method == "standardized":
        zu = zu / np.sqrt(var)[:, None]
    z[usable] = zu
    scale = float(np.cumsum(var)[-1]) if var.size else 0.0
    return usable, p, z, scale, int(usable.sum())


def operands(code, z) -> np.ndarray:
    """Z [n][K]: {z0, z1, z2, 0}[code]."""
    table = np.concatenate([z, np.zeros((z.shape[0], 1))], axis=1)  # [K][4]
    return np.ascontiguousarray(np.take_along_axis(table, code.astype(np.int64), axis=1).T)


def products(code, method="standardized", swap_hom=False, missing_as_het=False):
    """(S = Z Z^T, |Z| |Z|^T, Z, usable, z, scale, n_usable).  swap_hom / missing_as_het: what a class-confused kernel would compute - the
    values stay the true ones, the codes are misread."""
    c, a = counts(code)
    usable, _, z, scale, m = values(c, a, method)
    read = code.copy()
    if swap_hom:
        read = np.where(code == 0, 2, np.where(code == 2, 0, code)).astype(np.uint8)
    if missing_as_het:
        read = np.where(code == 3, 1, read).astype(np.uint8)
    Z = operands(read, z)
    return Z @ Z.T, np.abs(Z) @ np.abs(Z).T, Z, usable, z, scale, m


def bound(absprod, m_terms):
    """Any summation order of m f64 products is within (m + 2) 2^-53 sum |z_i| |z_j| of the exact value (tests/test_gpu_pca.py derives it);
    numpy's own sum has the same bound, so twice that separates the two."""
    return 2.0 * (m_terms + 2) * EPS * absprod


def pair_sites(code, usable) -> np.ndarray:
    called = (code[usable] <= 2).astype(np.uint64)
    return (called.T @ called).astype(np.uint64)


def matrix(S, N, method, denominator, n_usable, scale) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        if denominator == "pairs":
            assert method == "standardized"
            return np.where(N == 0, np.nan, S / N.astype(np.float64))
        return S / (np.float64(n_usable) if method == "standardized" else np.float64(scale))


def brute(code, method="standardized"):
    """(S, N) by a triple loop over plain Python floats."""
    K, n = code.shape
    c, a = counts(code)
    usable, _, z, _, _ = values(c, a, method)
    S, N = np.zeros((n, n)), np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            s, cnt = 0.0, 0
            for k in range(K):
                gi, gj = int(code[k, i]), int(code[k, j])
                if not usable[k] or gi > 2 or gj > 2:
                    continue
                s += float(z[k, gi]) * float(z[k, gj])
                cnt += 1
            S[i, j], N[i, j] = s, cnt
    return S, N


def fix_signs(v) -> np.ndarray:
    """Each column's component of the largest magnitude made positive (the lowest index on a tie)."""
    out = np.array(v, dtype=np.float64, copy=True)
    for k in range(out.shape[1]):
        at = int(np.argmax(np.abs(out[:, k])))  # argmax returns the first of equal maxima
        if out[at, k] < 0:
            out[:, k] = -out[:, k]
    return out


def eigen_pair(A, Z, m, k):
    """(eigenvalues descending [k], eigenvectors [n][k] by eigh(A), the same by the thin SVD of Z / sqrt(m), d0 = their largest
    disagreement).  Valid for A = Z Z^T / m (standardized, denominator sites)."""
    w, u = np.linalg.eigh(A)
    order = np.argsort(-w, kind="stable")
    w, u = w[order], u[:, order]
    a = fix_signs(u[:, :k])
    us, s, _ = np.linalg.svd(Z / np.sqrt(float(m)), full_matrices=False)
    b = fix_signs(us[:, :k])
    return w[:k], a, b, float(np.abs(a - b).max()), w


# ---- the seeded cohort of ferromic_amd/csrc/grm_host_check.cpp, and its checksum --------------------------------------------------------------
class SplitMix64:
    def __init__(self, seed):
        self.state = seed & MASK64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


def check_cohort(seed, K, n) -> np.ndarray:
    r = SplitMix64(seed)
    d = np.zeros((K, n), dtype=np.uint8)
    for k in range(K):
        t, gaps = r.next() % 17, r.next() % 32
        for s in range(n):
            g = int(r.next() % 16 < t) + int(r.next() % 16 < t)
            if gaps == 0 or (gaps < 4 and r.next() % 4 == 0):
                g = 3
            d[k, s] = g
    return d


def bits_of(v) -> int:
    v = np.float64(v)
    return 0x7FF8000000000000 if np.isnan(v) else int(v.view(np.uint64))


def checksum(code, method, denominator, S):
    """The checksum line's number for products S (the twin's: its bits are the twin's summation order, which the caller supplies)."""
    c, a = counts(code)
    usable, p, z, scale, m = values(c, a, method)
    N = pair_sites(code, usable)
    A = matrix(S, N, method, denominator, m, scale)
    n = code.shape[1]
    diag = fix_signs((-np.diag(A)).reshape(n, 1))[:, 0]
    h = (m * 1000003 + bits_of(scale)) & MASK64
    for k in range(code.shape[0]):
        h += (int(usable[k]) + 1) * ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) + bits_of(p[k]) * (2 * k + 1)
        h += bits_of(z[k, 0]) * 3 + bits_of(z[k, 1]) * 5 + bits_of(z[k, 2]) * 7
        h &= MASK64
    Sf, Nf, Af = S.reshape(-1), N.reshape(-1), A.reshape(-1)
    for e in range(n * n):
        h += bits_of(Sf[e]) * (2 * e + 1) + int(Nf[e]) * ((0xBF58476D1CE4E5B9 + e) & MASK64) + bits_of(Af[e]) * (2 * e + 3)
        h &= MASK64
    for i in range(n):
        h = (h + bits_of(diag[i]) * (4 * i + 1)) & MASK64
    return h, m
