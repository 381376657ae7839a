"""The IBD-segment oracle, written from the definition in include/ferromic_hip.h (fmh_ibd_scan) as an explicit loop over the kept rows that
carries the state of every pair (run open or not, its first row, its missing count) in plain arrays.  No words, no blocks, no stitch: it
shares nothing with the kernels or the host twin.  Also the cohort generators of the IBD tests: uniform random genotypes give only runs of
a few rows (kept as the many-short-runs background), so sharing is PLANTED: founder genotype tracks are copied over stretches."""

import numpy as np

IBD1, IBD2 = 1, 2
NOT_CALLED = 3
NO_LIMIT = 0xFFFFFFFF
TABLES = ("n_segments", "sum_sites", "sum_length", "longest_length")


def params(mode=IBD1, min_sites=436, min_length=7_000_000, max_gap=1_000_000, max_bp_per_site=0, max_missing=None):
    return dict(mode=mode, min_sites=min_sites, min_length=min_length, max_gap=max_gap or 0, max_bp_per_site=max_bp_per_site or 0,
                max_missing=NO_LIMIT if max_missing is None else max_missing)


def dosages(x, called, samples=None):
    """[rows][n] uint8 dosage table (0, 1, 2; 3 = not called) of diploid samples from alleles x [rows][2 S] and called [rows][2 S] (or
    None): a genotype is called iff both entries are called and both alleles are <= 1."""
    x = np.asarray(x)
    a, b = x[:, 0::2].astype(np.int64), x[:, 1::2].astype(np.int64)
    ok = (a <= 1) & (b <= 1)
    if called is not None:
        ok &= called[:, 0::2] & called[:, 1::2]
    d = np.where(ok, a + b, NOT_CALLED).astype(np.uint8)
    return d if samples is None else d[:, np.asarray(samples, dtype=np.int64)]


def pair_states(d_row, mode):
    """(disc [n][n], miss [n][n]) of one kept row's dosages."""
    d = d_row.astype(np.int64)
    ok = d < NOT_CALLED
    both = ok[:, None] & ok[None, :]
    if mode == IBD1:
        disc = both & (np.abs(d[:, None] - d[None, :]) == 2)
    else:
        disc = both & (d[:, None] != d[None, :])
    return disc, ~both


def scan(dosage, x, p):
    """The definition over a dosage table [K][n] and positions x [K] (None: x = k).  Returns a dict: the four tables as uint64 [n][n]
    (both triangles, diagonal 0), `segments` = the qualifying runs as sorted tuples (a, b, n_sites, n_missing, first, last), `runs` = EVERY
    maximal run as (a, b, first, last, n_missing, length, qualifies), `breaks` [K] bool and `n_disc` [n][n] = the pairs' DISC rows."""
    dosage = np.asarray(dosage, dtype=np.uint8)
    K, n = dosage.shape
    x = np.arange(K, dtype=np.int64) if x is None else np.asarray(x, dtype=np.int64)
    breaks = np.zeros(K, dtype=bool)
    for k in range(1, K):
        breaks[k] = p["max_gap"] > 0 and int(x[k]) - int(x[k - 1]) > p["max_gap"]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    is_open = np.zeros((n, n), dtype=bool)
    first = np.zeros((n, n), dtype=np.int64)
    missing = np.zeros((n, n), dtype=np.int64)
    n_disc = np.zeros((n, n), dtype=np.int64)
    ended = []  # (a, b, first, last, n_missing) arrays, one entry per kept row at which runs ended

    def close(which, last):
        a, b = np.nonzero(which)
        if a.size:
            ended.append((a, b, first[which], np.full(a.size, last, dtype=np.int64), missing[which]))
        is_open[which] = False

    for k in range(K):
        disc, miss = pair_states(dosage[k], p["mode"])
        disc &= upper
        n_disc += disc
        close(is_open & (disc | breaks[k]), k - 1)
        start = upper & ~disc & ~is_open
        first[start] = k
        missing[start] = 0
        is_open |= start
        missing += is_open & miss
    if K:
        close(is_open.copy(), K - 1)

    out = {name: np.zeros((n, n), dtype=np.uint64) for name in TABLES}
    segments, runs = [], []
    for a_, b_, f_, l_, m_ in ended:
        for a, b, f, l, m in zip(a_.tolist(), b_.tolist(), f_.tolist(), l_.tolist(), m_.tolist()):
            n_sites = l - f + 1
            length = int(x[l]) - int(x[f]) + 1
            ok = (n_sites >= p["min_sites"] and length >= p["min_length"] and m <= p["max_missing"]
                  and (p["max_bp_per_site"] == 0 or length <= p["max_bp_per_site"] * n_sites))
            runs.append((a, b, f, l, m, length, ok))
            if not ok:
                continue
            for i, j in ((a, b), (b, a)):
                out["n_segments"][i, j] += 1
                out["sum_sites"][i, j] += n_sites
                out["sum_length"][i, j] += length
                out["longest_length"][i, j] = max(int(out["longest_length"][i, j]), length)
            segments.append((a, b, n_sites, m, f, l))
    out.update(segments=sorted(segments, key=lambda s: (s[0], s[1], s[4])), runs=runs, breaks=breaks, n_disc=n_disc + n_disc.T)
    return out


def segment_tuples(seg):
    """A structured segment array (ferromic_amd.device.IBD_SEGMENT_DTYPE) as the oracle's sorted tuples."""
    rows = [(int(s["a"]), int(s["b"]), int(s["n_sites"]), int(s["n_missing"]), int(s["first_row"]), int(s["last_row"])) for s in seg]
    return sorted(rows, key=lambda s: (s[0], s[1], s[4]))


def checksum(result):
    """What ferromic_amd/csrc/ibd_host_check.cpp prints for a scan: an order-free hash of the tables and segments."""
    mask = (1 << 64) - 1
    h = 0
    for name in TABLES:
        for i, v in enumerate(result[name].reshape(-1).tolist()):
            h = (h + (int(v) + 1) * (0x9E3779B97F4A7C15 * (i + 1) & mask)) & mask
        h = (h * 31 + 7) & mask
    for s in result["segments"]:
        e = 0
        for v in s:
            e = (e * 1000003 + int(v) + 1) & mask
        h = (h + e * e) & mask
    return h


# ---- cohorts ----------------------------------------------------------------------------------------------------------------------------
def planted_dosages(K, n, seed, short=False, miss=0.02, founders=3):
    """[K][n] uint8 dosages.  Founder tracks of genotypes; per sample alternating stretches: an exact copy of a founder (two samples that
    copy the same founder over the same rows are IBD2 there), a copy with a third of its homozygotes made heterozygous (compatible with the
    founder's copies under IBD1, not under IBD2), or fresh genotypes (the many-short-runs background).  Stretches of 15..70 rows, or 3..9
    with short=True.  Samples 0 and 1 (n > 2) copy founder 0 over EVERY row: one run over everything.  A share `miss` is not called."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.2, 0.8, size=K)
    tracks = (rng.random((founders, K)) < freq).astype(np.uint8) + (rng.random((founders, K)) < freq).astype(np.uint8)
    lo, hi = (3, 9) if short else (15, 70)
    d = np.zeros((K, n), dtype=np.uint8)
    for i in range(n):
        k = 0
        while k < K:
            length = min(int(rng.integers(lo, hi + 1)), K - k)
            kind = int(rng.integers(0, 3))
            f = int(rng.integers(0, founders))
            fresh = (rng.random(length) < freq[k:k + length]).astype(np.uint8) + (rng.random(length) < freq[k:k + length]).astype(np.uint8)
            if kind == 0:
                part = tracks[f, k:k + length].copy()
            elif kind == 1:
                part = tracks[f, k:k + length].copy()
                part[(part != 1) & (rng.random(length) < 1 / 3)] = 1
            else:
                part = fresh
            d[k:k + length, i] = part
            k += length
    if n > 2:
        d[:, 0] = tracks[0]
        d[:, 1] = tracks[0]
    d[rng.random((K, n)) < miss] = NOT_CALLED
    return d


def uniform_dosages(K, n, seed, miss=0.02):
    """Independent genotypes at allele frequency one half: runs of a few rows only."""
    rng = np.random.default_rng(seed + 5)
    d = (rng.integers(0, 2, size=(K, n)) + rng.integers(0, 2, size=(K, n))).astype(np.uint8)
    d[rng.random((K, n)) < miss] = NOT_CALLED
    return d


def planted_positions(K, seed, step=(1, 2000), jumps=4, jump=5_000_000):
    """K ascending positions with a few jumps of `jump` (above the default max_gap) and some repeated positions."""
    rng = np.random.default_rng(seed + 17)
    d = rng.integers(step[0], step[1] + 1, size=K).astype(np.int64)
    d[rng.random(K) < 0.02] = 0
    if K > 3:
        d[rng.choice(np.arange(1, K), size=min(jumps, K - 1), replace=False)] = jump
    if K:
        d[0] = int(rng.integers(0, 1000))
    return np.cumsum(d)


def genotypes_from_dosages(d, seed, columns=None, high_allele=1, uncalled=True):
    """Alleles [K][2 S] uint8 and called [K][2 S] bool that realise the dosages: 0 as 0/0, 2 as 1/1, 1 as 0/1 or 1/0, NOT_CALLED as an
    uncalled entry (one or both, over random alleles) or - half of the time, when high_allele > 1 - a called allele above 1 (always, with
    uncalled=False: the matrix has no called plane; called is then all True).  `columns` (S >= n) pads further samples with random
    genotypes."""
    assert uncalled or high_allele > 1 or not (d == NOT_CALLED).any(), "a missing genotype needs an uncalled entry or an allele above 1"
    rng = np.random.default_rng(seed + 29)
    K, n = d.shape
    S = n if columns is None else columns
    full = np.zeros((K, S), dtype=np.uint8)
    full[:, :n] = d
    if S > n:
        full[:, n:] = rng.integers(0, 4 if (uncalled or high_allele > 1) else 3, size=(K, S - n))
    coin = rng.integers(0, 2, size=(K, S)).astype(np.uint8)
    a = np.where(full == 2, 1, np.where(full == 1, coin, 0)).astype(np.uint8)
    b = np.where(full == 2, 1, np.where(full == 1, 1 - coin, 0)).astype(np.uint8)
    missing = full == NOT_CALLED
    a = np.where(missing, rng.integers(0, 2, size=(K, S)), a).astype(np.uint8)
    b = np.where(missing, rng.integers(0, 2, size=(K, S)), b).astype(np.uint8)
    called_a = np.ones((K, S), dtype=bool)
    called_b = np.ones((K, S), dtype=bool)
    by_allele = missing & ((rng.random((K, S)) < 0.5) | (not uncalled)) & (high_allele > 1)
    side = rng.integers(0, 3, size=(K, S))                    # which entries of an uncalled genotype are uncalled: a, b or both
    called_a[missing & ~by_allele & (side != 1)] = False
    called_b[missing & ~by_allele & (side != 0)] = False
    high = rng.integers(2, max(high_allele, 2) + 1, size=(K, S)).astype(np.uint8)
    a = np.where(by_allele & (side != 1), high, a).astype(np.uint8)
    b = np.where(by_allele & (side == 1), high, b).astype(np.uint8)
    x = np.empty((K, 2 * S), dtype=np.uint8)
    x[:, 0::2], x[:, 1::2] = a, b
    called = np.empty((K, 2 * S), dtype=bool)
    called[:, 0::2], called[:, 1::2] = called_a, called_b
    return x, called
