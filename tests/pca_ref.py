"""numpy f64 restatement of the reference's haplotype PCA (src/pca.rs) - the oracle of the PCA tests.

Cites are to the reference's src/pca.rs.  Nothing here touches the device or the library under test.
"""

from __future__ import annotations

import numpy as np

# efficient_pca::pca::NEAR_ZERO_THRESHOLD (pca.rs:2).  Its value could not be verified; no test may depend on it: every kept site has
# a standard deviation far above it and every tested component an eigenvalue far above it.
NEAR_ZERO_THRESHOLD = 1e-9


def site_filter(genotypes: np.ndarray, variant_rule: bool = False):
    """compute_chromosome_pca_from_dense (pca.rs:257-290) or, with variant_rule, compute_chromosome_pca (:68-125) on a
    (variants, samples, 2) integer array with negative = missing.  Returns (kept row indices, complete_count).

    The two count differently: on dense input a site with an allele above 1 is not complete (:261-268); on Variant input it is (:93-117)
    and is skipped afterwards (:99-117)."""
    g = np.asarray(genotypes).astype(np.int64)
    v, s, p = g.shape
    assert p == 2
    n = s * 2
    flat = g.reshape(v, n)
    missing = (flat < 0).any(axis=1)
    high = (flat > 1).any(axis=1)
    complete = ~missing if variant_rule else ~missing & ~high
    candidates = np.nonzero(~missing & ~high)[0]
    allele_sum = flat[candidates].sum(axis=1)
    freq = allele_sum.astype(np.float64) / float(n)  # :284 allele_sum as f64 / n_haplotypes as f64
    maf = np.minimum(freq, 1.0 - freq)               # :285
    kept = candidates[maf >= 0.05]                   # :286
    return np.array(kept, dtype=np.int64), int(complete.sum())


def clamp_components(requested: int, complete_count: int, n_haplotypes: int) -> int:
    """pca.rs:333-334"""
    return min(requested, min(complete_count, n_haplotypes))


def haplotype_matrix(genotypes: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """pca.rs:369-408: rows = haplotypes (sample * 2 + side), columns = kept sites, f64."""
    g = np.asarray(genotypes)
    v, s, _ = g.shape
    return np.ascontiguousarray(g.reshape(v, s * 2)[kept].T.astype(np.float64))


def standardize(x: np.ndarray) -> np.ndarray:
    """pca.rs:579-662: column mean, variance over n - 1, scale 1 when the deviation is numerically zero."""
    mean = x.mean(axis=0)
    var = x.var(axis=0, ddof=1)
    var = np.where(np.isfinite(var), np.maximum(var, 0.0), 0.0)
    sd = np.sqrt(var)
    sd = np.where(~np.isfinite(sd) | (sd <= NEAR_ZERO_THRESHOLD), 1.0, sd)
    return (x - mean) * (1.0 / sd)


def set_clear_values(alt_counts: np.ndarray, n: int):
    """What a set / a clear bit of a kept site stands for after standardize(): ((1 - mean) / sd, -mean / sd) from the integer count."""
    c = np.asarray(alt_counts, dtype=np.float64)
    mean = c / float(n)
    var = (c * (1.0 - mean) ** 2 + (float(n) - c) * mean ** 2) / float(n - 1)
    sd = np.sqrt(var)
    sd = np.where(sd <= NEAR_ZERO_THRESHOLD, 1.0, sd)
    return (1.0 - mean) / sd, (0.0 - mean) / sd


def gram(z: np.ndarray) -> np.ndarray:
    """pca.rs:734-746"""
    return z @ z.T / float(z.shape[0] - 1)


def transform(x: np.ndarray, n_components: int):
    """fast_exact_pca_transform (pca.rs:541-803) through the Gram branch (:733-800) for every shape: (scores, eigenvalues descending).

    The reference takes the covariance branch (:667-732) when features <= haplotypes; that gives the same scores up to the sign of a
    column, and `kept = min(n_components, min(features, haplotypes))` columns (:694, :759)."""
    n, m = x.shape
    z = standardize(x.copy())
    w, u = np.linalg.eigh(gram(z))
    order = np.argsort(-w, kind="stable")
    w, u = w[order], u[:, order]
    kept = min(n_components, min(m, n))
    scores = np.zeros((n, kept))
    for k in range(kept):
        lam = max(w[k], 0.0) if np.isfinite(w[k]) else 0.0
        if lam <= NEAR_ZERO_THRESHOLD:
            continue
        sigma = np.sqrt(float(n - 1) * lam)  # :781
        if not np.isfinite(sigma) or sigma <= NEAR_ZERO_THRESHOLD:
            continue
        scores[:, k] = u[:, k] * sigma  # :794-796
    return scores, w


def transform_svd(x: np.ndarray, n_components: int) -> np.ndarray:
    """The independent route: scores = U S of the thin SVD of the standardised matrix."""
    z = standardize(x.copy())
    u, s, _ = np.linalg.svd(z, full_matrices=False)
    kept = min(n_components, min(x.shape))
    return u[:, :kept] * s[:kept]


def canonical_signs(scores: np.ndarray) -> np.ndarray:
    """Each column's first entry with |v| > 1e-12 made positive (the reference's PCA pybench does the same before it compares)."""
    out = np.array(scores, dtype=np.float64, copy=True)
    for k in range(out.shape[1]):
        big = np.nonzero(np.abs(out[:, k]) > 1e-12)[0]
        if big.size and out[big[0], k] < 0:
            out[:, k] = -out[:, k]
    return out


def chromosome_pca(genotypes: np.ndarray, positions, sample_names, n_components: int, variant_rule: bool = False):
    """(labels, coordinates, positions) as ChromosomePcaResult holds them (pca.rs:415-479, lib.rs:196-257)."""
    kept, complete = site_filter(genotypes, variant_rule)
    if kept.size == 0:
        raise ValueError('VCF error: Parse("No variants with MAF >= 5% found for PCA")')
    n = np.asarray(genotypes).shape[1] * 2
    scores, _ = transform(haplotype_matrix(genotypes, kept), clamp_components(n_components, complete, n))
    labels = [f"{name}_{side}" for name in sample_names for side in ("L", "R")]
    return labels, scores, np.asarray(positions, dtype=np.int64)[kept]


def tsv_text(labels, coordinates: np.ndarray) -> str:
    """write_chromosome_pca_to_file, pca.rs:859-880"""
    lines = ["Haplotype" + "".join(f"\tPC{k + 1}" for k in range(coordinates.shape[1]))]
    for label, row in zip(labels, coordinates):
        lines.append(label + "".join(f"\t{v:.6f}" for v in row))
    return "\n".join(lines) + "\n"


def pybench_cohort(variants: int, samples: int, seed: int, scale: float = 0.05, populations: int = 2) -> np.ndarray:
    """The reference's benchmark recipe (base frequency ~ Beta(0.8, 0.8), per-population divergence ~ N(0, scale), clipped) as an
    int8 (variants, samples, 2) array, samples split evenly over `populations`."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=variants)
    blocks = []
    per = samples // populations
    for p in range(populations):
        count = per if p < populations - 1 else samples - per * (populations - 1)
        freq = np.clip(base + rng.normal(0.0, scale, size=variants), 0.001, 0.999)
        blocks.append(rng.binomial(1, freq[:, None], size=(variants, count * 2)).astype(np.int8).reshape(variants, count, 2))
    return np.concatenate(blocks, axis=1)
