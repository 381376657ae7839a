"""The LD-clumping oracle, written from the definition in include/ferromic_hip.h (fmh_clump, fmh_geno_ld_pairs): counts from a dosage table by
boolean indexing and Python-int sums, r^2 as one Python float expression, rule 3 as a plain loop over candidates sorted by (p, row).  No
bit planes, no tiles, no partner ranges: it shares nothing with the kernels or the host twin.  Also the cohorts of the clumping tests - a
founder mosaic, so that neighbouring sites are in LD - and the splitmix64 cohort and checksum of ferromic_amd/csrc/clump_host_check.cpp."""

import math
import struct

import numpy as np

NOT_CALLED = 3
NONE = -1
COUNTS = ("n", "sum_a", "sum_b", "sq_a", "sq_b", "cross")


def params(p1=1e-4, p2=1e-2, r2=0.5, window=250_000):
    return dict(p1=float(p1), p2=float(p2), r2=float(r2), window=int(window))


def counts(a, b):
    """(n, sum_a, sum_b, sq_a, sq_b, cross) of two dosage rows as Python ints, over the samples called at both."""
    a, b = np.asarray(a), np.asarray(b)
    both = (a < NOT_CALLED) & (b < NOT_CALLED)
    ga, gb = [int(v) for v in a[both]], [int(v) for v in b[both]]
    return (len(ga), sum(ga), sum(gb), sum(v * v for v in ga), sum(v * v for v in gb), sum(u * v for u, v in zip(ga, gb)))


def r2_of(c):
    n, sum_a, sum_b, sq_a, sq_b, cross = (int(v) for v in c)
    cov, va, vb = n * cross - sum_a * sum_b, n * sq_a - sum_a * sum_a, n * sq_b - sum_b * sum_b
    if va == 0 or vb == 0:
        return math.nan
    return float(cov) * float(cov) / (float(va) * float(vb))


def pair_counts(dosage, rows_a, rows_b):
    """int64 [P][6] of the row pairs of a dosage table."""
    return np.array([counts(dosage[a], dosage[b]) for a, b in zip(rows_a, rows_b)], dtype=np.int64).reshape(-1, 6)


def clump(dosage, x, p, prm):
    """The definition over a dosage table [K][n], positions x [K] (None: x = k) and p [K].  Returns a dict: index_of int64 [K] (-1 = none),
    r2 float64 [K] (NaN = none), indexes (rows in the order they were chosen), n_clumps, and what the tests' conditions ask about:
    claimed_before_turn (candidates skipped because an earlier index owned them) and unassigned (participants no index claimed)."""
    dosage = np.asarray(dosage, dtype=np.uint8)
    K = dosage.shape[0]
    x = [int(v) for v in (np.arange(K) if x is None else x)]
    p = [float(v) for v in p]
    participant = [not math.isnan(p[k]) and p[k] <= prm["p2"] for k in range(K)]
    candidates = sorted((p[k], k) for k in range(K) if participant[k] and p[k] <= prm["p1"])
    index_of = [NONE] * K
    r2 = [math.nan] * K
    indexes, skipped = [], 0
    for _, i in candidates:
        if index_of[i] != NONE:
            skipped += 1
            continue
        index_of[i] = i
        r2[i] = r2_of(counts(dosage[i], dosage[i]))
        indexes.append(i)
        for j in range(K):
            if j == i or not participant[j] or index_of[j] != NONE or abs(x[j] - x[i]) > prm["window"]:
                continue
            v = r2_of(counts(dosage[i], dosage[j]))
            if v >= prm["r2"]:  # False for NaN
                index_of[j] = i
                r2[j] = v
    unassigned = sum(1 for k in range(K) if participant[k] and index_of[k] == NONE)
    return dict(index_of=np.array(index_of, dtype=np.int64).reshape(K), r2=np.array(r2, dtype=np.float64).reshape(K), indexes=indexes, n_clumps=len(indexes),
                claimed_before_turn=skipped, unassigned=unassigned, participants=int(sum(participant)), candidates=len(candidates))


def sizes(result):
    """members per clump (the index included), in the order of result['indexes']"""
    return [int((result["index_of"] == i).sum()) for i in result["indexes"]]


def same_bits(a, b):
    """float64 arrays equal bit for bit, every NaN alike"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.uint64(0x7FF8000000000000)
    ua, ub = np.where(np.isnan(a), nan, a.view(np.uint64)), np.where(np.isnan(b), nan, b.view(np.uint64))
    return a.shape == b.shape and bool(np.array_equal(ua, ub))


# ---- cohorts ----------------------------------------------------------------------------------------------------------------------------
def mosaic_dosages(K, n, seed, miss=0.04, founders=4, stretch=(10, 50), flip=0.02):
    """[K][n] uint8 dosages with LD: founder haplotype tracks; each of a sample's two haplotypes copies a founder over stretches of rows
    (a share `flip` of the copied alleles flipped), so neighbouring rows are correlated and far rows are not.  Row 1 duplicates row 0 and
    row 2 complements it (g -> 2 - g) when K > 3, rows K - 1 and K - 2 are monomorphic (all 0; all 2) when K > 8.  A share `miss` of the
    genotypes is not called."""
    rng = np.random.default_rng(seed)
    tracks = (rng.random((founders, K)) < rng.uniform(0.15, 0.85, size=K)).astype(np.uint8)
    d = np.zeros((K, n), dtype=np.uint8)
    for i in range(n):
        for _ in range(2):
            k = 0
            while k < K:
                length = min(int(rng.integers(stretch[0], stretch[1] + 1)), K - k)
                part = tracks[int(rng.integers(0, founders)), k:k + length].copy()
                part ^= (rng.random(length) < flip).astype(np.uint8)
                d[k:k + length, i] += part
                k += length
    if K > 3:
        d[1] = d[0]
        d[2] = 2 - d[0]
    if K > 8:
        d[K - 1] = 0
        d[K - 2] = 2
    d[rng.random((K, n)) < miss] = NOT_CALLED
    if K > 3 and miss > 0:  # the duplicate and the complement are called where their model is: r^2 is exactly 1
        gone = d[0] == NOT_CALLED
        d[1] = np.where(gone, NOT_CALLED, d[0])
        d[2] = np.where(gone, NOT_CALLED, 2 - d[0])
    return d


def mosaic_positions(K, seed, step=(0, 3)):
    """K non-decreasing positions with repeated ones (steps of step[0] .. step[1])."""
    rng = np.random.default_rng(seed + 17)
    return np.cumsum(rng.integers(step[0], step[1] + 1, size=K)).astype(np.int64)


def mosaic_p(K, seed, top=0.12, nan=0.02, zero=0.02):
    """K p values on a grid of 1/4096 steps below `top` (many ties), a share exactly 0 and a share NaN."""
    rng = np.random.default_rng(seed + 41)
    p = rng.integers(0, 4096, size=K) / 4096.0 * top
    u = rng.random(K)
    p[u < zero] = 0.0
    p[(u >= zero) & (u < zero + nan)] = np.nan
    return p


# ---- the stand-alone program's cohort and checksum ------------------------------------------------------------------------------------------
MASK64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.state = seed & MASK64

    def __call__(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


def splitmix_cohort(seed, K, n):
    """(dosage [K][n], x [K], p [K]) as ferromic_amd/csrc/clump_host_check.cpp draws them."""
    rnd = SplitMix64(seed)
    F = 4
    founder = [[rnd() % 2 for _ in range(K)] for _ in range(F)]
    d = np.zeros((K, n), dtype=np.uint8)
    for i in range(n):
        for _ in range(2):
            k = 0
            while k < K:
                length, src = 10 + rnd() % 40, rnd() % F
                j = 0
                while j < length and k < K:
                    r = rnd() % 100
                    d[k, i] += (1 - founder[src][k]) if r < 2 else founder[src][k]
                    j += 1
                    k += 1
    flat = d.reshape(-1)
    for i in range(K * n):
        if rnd() % 100 < 3:
            flat[i] = NOT_CALLED
    x = np.zeros(K, dtype=np.int64)
    for k in range(K):
        x[k] = (x[k - 1] if k else 0) + rnd() % 4
    p = np.zeros(K, dtype=np.float64)
    for k in range(K):
        r = rnd() % 1000
        p[k] = math.nan if r < 20 else 0.0 if r < 40 else (rnd() % 4096) / 40960.0
    return d, x, p


def checksum(dosage, result):
    """What clump_host_check prints for a clumping: an order-free hash of the assignment, the r^2 bits and the owned rows' counts."""
    K = dosage.shape[0]
    h = result["n_clumps"]
    for k in range(K):
        v = float(result["r2"][k])
        bits = 0x7FF8000000000000 if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", v))[0]
        index = 0xFFFFFFFF if result["index_of"][k] == NONE else int(result["index_of"][k])
        h = (h + (index + 1) * ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) + bits * (2 * k + 1)) & MASK64
    owned = 0
    for k in range(K):
        i = int(result["index_of"][k])
        if i == NONE:
            continue
        owned += 1
        e = 0
        for v in (k,) + counts(dosage[i], dosage[k]):
            e = (e * 1000003 + int(v) + 1) & MASK64
        h = (h + e * e) & MASK64
    return h, owned
