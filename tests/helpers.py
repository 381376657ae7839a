"""Shared builders for parity tests: random cohorts in the reference's data model plus the
oracle-side expectations, so GPU tests read like the reference's own tests."""

from __future__ import annotations

import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import dense as D
from oracle import ferromic_ref as R


def random_sparse_variants(rng: random.Random, n_sites: int, n_samples: int, max_allele: int = 1,
                           p_missing: float = 0.0, p_haploid: float = 0.0, all_missing_rows: int = 0):
    """Variants in the sparse model (None = missing sample, 1-allele genotype = haploid call)."""
    rows = []
    pos = 0
    for s in range(n_sites):
        pos += rng.randint(1, 49)
        freq = [rng.random() for _ in range(max_allele + 1)]
        tot = sum(freq)
        cum = np.cumsum([f / tot for f in freq])

        def draw():
            u = rng.random()
            return int(np.searchsorted(cum, u, side="right").clip(0, max_allele))

        row = []
        for i in range(n_samples):
            if s < all_missing_rows or rng.random() < p_missing:
                row.append(None)
            elif rng.random() < p_haploid:
                row.append([draw()])
            else:
                row.append([draw(), draw()])
        rows.append((pos, row))
    return [R.make_variant(p, g) for p, g in rows]


def dense_from_variants(variants, n_samples) -> R.DenseGenotypeMatrix:
    m = R.DenseGenotypeMatrix.from_variants(variants, n_samples)
    assert m is not None
    return m


def random_dense_matrix(rng: np.random.Generator, n_sites: int, n_samples: int, ploidy: int = 2,
                        max_allele: int = 1, p_missing: float = 0.0) -> R.DenseGenotypeMatrix:
    """A dense matrix in the reference host layout (per-allele missing bits, like from_numpy)."""
    H = n_samples * ploidy
    freq = rng.beta(0.8, 0.8, size=(n_sites, 1))
    if max_allele <= 1:
        data = (rng.random((n_sites, H)) < freq).astype(np.uint8)
    else:
        data = rng.integers(0, max_allele + 1, size=(n_sites, H), dtype=np.uint8)
        data[rng.random((n_sites, H)) < 0.6] = 0
        data[0, 0] = max_allele
    missing = None
    if p_missing > 0:
        miss = rng.random((n_sites, H)) < p_missing
        data[miss] = 0
        bits = np.packbits(miss.reshape(-1), bitorder="little")
        pad = (-len(bits)) % 8
        words = np.frombuffer(np.concatenate([bits, np.zeros(pad, np.uint8)]).tobytes(), dtype="<u8")
        missing = [int(w) for w in words]
    return R.DenseGenotypeMatrix(bytes(data.reshape(-1)), missing, n_sites, n_samples, ploidy, int(data.max()) if n_sites else 0)


def missing_words_np(m: R.DenseGenotypeMatrix) -> Optional[np.ndarray]:
    return None if m.missing is None else np.array(m.missing, dtype=np.uint64)


def haps_for_samples(samples: Sequence[int]) -> List[Tuple[int, int]]:
    return [(s, side) for s in samples for side in (0, 1)]


def opt(x: Optional[float]) -> float:
    return float("nan") if x is None else x


def assert_bits_equal(actual: np.ndarray, expected: Sequence[float], what: str):
    exp = np.array(expected, dtype=np.float64)
    a = np.asarray(actual, dtype=np.float64)
    assert a.shape == exp.shape, what
    both_nan = np.isnan(a) & np.isnan(exp)
    same = (a.view(np.uint64) == exp.view(np.uint64)) | both_nan  # the sign of a zero counts: +0.0 and -0.0 are different bits
    if not same.all():
        i = int(np.argmin(same))
        raise AssertionError(f"{what}: first mismatch at {i}: gpu={a[i]!r} oracle={exp[i]!r}")


def rel_close(a: float, b: float, rel: float = 1e-9, abs_tol: float = 1e-12) -> bool:
    """north_star tolerance: 1e-9 relative (1e-12 absolute near zero)."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return math.isclose(a, b, rel_tol=rel, abs_tol=abs_tol)


def assert_close_rel(actual: np.ndarray, expected: Sequence[float], what: str, rel: float = 1e-12):
    exp = np.array(expected, dtype=np.float64)
    a = np.asarray(actual, dtype=np.float64)
    assert a.shape == exp.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(exp)), f"{what}: None pattern differs"
    ok = np.isnan(a) | np.isclose(a, exp, rtol=rel, atol=1e-15)
    if not ok.all():
        i = int(np.argmin(ok))
        raise AssertionError(f"{what}: first mismatch at {i}: gpu={a[i]!r} oracle={exp[i]!r}")


# ---- host cohorts for the full-scale oracle gates (tests/test_gpu_scale_general.py, tests/test_gpu_scale_sparse.py) ----


def thresholds(S, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=S)
    div = rng.normal(0.0, sigma, size=S)
    return (np.stack([np.clip(base + div, 0.001, 0.999), np.clip(base - div, 0.001, 0.999)]) * (1 << 24)).astype(np.uint32)


def pick_rows(rng, S, frac):
    """A seeded set of rows that always holds the first and the last row and rows on both sides of 64-row tile edges."""
    edges = np.array([63, 64, 127, 128, 64 * (S // 128) - 1, 64 * (S // 128), 64 * (S // 64) - 1], dtype=np.int64)
    rows = np.concatenate([[0, S - 1], edges[edges < S], rng.choice(S, size=max(1, int(frac * S)), replace=False)])
    return np.unique(rows)


def set_missing(words, Hc, rows, cols):
    idx = rows.astype(np.uint64) * np.uint64(Hc) + cols.astype(np.uint64)
    np.bitwise_or.at(words, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))


def build_cohort(S, N, seed, frac_multi, max_allele, frac_gap, cut):
    """Host bytes [S][2N] and missing words (or None).  Population 1 = samples [0, cut), population 2 = [cut, N - 1).  Among the multi-allelic
    rows, some are built for the first-occurrence cases of the general D_xy: the two populations meet their alleles in different orders,
    either one has fewer distinct alleles, a tie; among the gap rows, a missing call at a population's first member, a population with
    one called haplotype and one with none."""
    Hc = 2 * N
    rng = np.random.default_rng(seed)
    poc = np.repeat((np.arange(N) >= N // 2).astype(np.uint8), 2)
    data, _ = D.generate(S, Hc, seed, 0, thresholds(S, seed), poc, 0, 16)
    data = data.reshape(S, Hc)
    c1, c2 = np.arange(0, 2 * cut), np.arange(2 * cut, Hc - 2)
    multi = np.zeros(0, dtype=np.int64)
    if frac_multi > 0:
        multi = pick_rows(rng, S, frac_multi)
        sub = data[multi]
        vals = rng.integers(0, max_allele + 1, size=sub.shape, dtype=np.uint8)
        sub = np.where(rng.random(sub.shape) < 0.5, sub, vals)
        sub[np.arange(len(multi)), rng.integers(0, Hc, size=len(multi))] = rng.integers(2, max_allele + 1, size=len(multi))
        data[multi] = sub
        for i, r in enumerate(multi[rng.permutation(len(multi))[:300]]):
            kind = i % 4
            k1 = int(rng.integers(3, max_allele + 2)) if kind != 1 else int(rng.integers(1, 3))
            k2 = int(rng.integers(3, max_allele + 2)) if kind != 2 else int(rng.integers(1, 3))
            if kind == 3:
                k2 = k1
            a1 = rng.permutation(max_allele + 1)[:k1]
            a2 = rng.permutation(max_allele + 1)[:k2] if kind != 3 else a1[::-1].copy()
            for cols, al in ((c1, a1), (c2, a2)):
                v = al[rng.integers(0, len(al), size=len(cols))]
                v[:len(al)] = al
                data[r, cols] = v
        data[multi[0], 0] = max_allele  # the declared max_allele is met
    words = None
    if frac_gap > 0:
        words = np.zeros((S * Hc + 63) // 64, dtype=np.uint64)
        gaps = pick_rows(rng, S, frac_gap)
        rr, cc = np.nonzero(rng.random((len(gaps), Hc)) < 0.05)
        rows, cols = [gaps[rr], gaps], [cc, rng.integers(0, Hc, size=len(gaps))]
        special = gaps[rng.permutation(len(gaps))[:200]]
        for i, r in enumerate(special):
            sel = (c1[:1], c2[:1], c1[1:], c2)[i % 4]  # first member of 1 / of 2; one called haplotype in 1; nothing called in 2
            rows.append(np.full(len(sel), r))
            cols.append(sel)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        data[rows, cols] = 0
        set_missing(words, Hc, rows, cols)
    return data, words, multi
