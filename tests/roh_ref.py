"""The runs-of-homozygosity oracle, written from the definition in include/ferromic_hip.h (fmh_roh_scan, fmh_roh_need) with explicit
loops: every window is enumerated one by one and counted from the state table, every row asks every window that covers it, every run is
walked row by row.  No histories, no blocks, no sliding counts: it shares nothing with the kernels or the host twin.  Also the cohort
generators of the ROH tests: uniform random genotypes hold no run and would test nothing, so stretches of homozygosity are PLANTED."""

import numpy as np

HOM, HET, MISS = 0, 1, 2
NO_LIMIT = 0xFFFFFFFF
TABLES = ("n_runs", "sum_sites", "sum_length", "longest_length")


def need_table(threshold, window):
    """need[c], c = 1..window: the smallest integer h >= 1 with float(h) >= threshold * float(c); 65 entries, the others 0."""
    need = [0] * 65
    for c in range(1, window + 1):
        want = float(threshold) * float(c)
        h = 1
        while not float(h) >= want:
            h += 1
        need[c] = h
    return need


def params(window=50, window_het=1, window_missing=5, threshold=0.05, min_sites=100, min_length=1_000_000, max_gap=1_000_000,
           max_bp_per_site=50_000, max_het=None, max_missing=None, bin_edges=()):
    return dict(window=window, window_het=window_het, window_missing=window_missing, threshold=threshold, need=need_table(threshold, window),
                min_sites=min_sites, min_length=min_length, max_gap=max_gap or 0, max_bp_per_site=max_bp_per_site or 0,
                max_het=NO_LIMIT if max_het is None else max_het, max_missing=NO_LIMIT if max_missing is None else max_missing,
                bin_edges=tuple(bin_edges or ()))


def states(x, called, samples=None):
    """[rows][n] uint8 state table of diploid samples from alleles x [rows][2 S] and called [rows][2 S] (or None): a genotype is called iff
    both entries are called and both alleles are <= 1."""
    x = np.asarray(x)
    a, b = x[:, 0::2].astype(np.int64), x[:, 1::2].astype(np.int64)
    ok = (a <= 1) & (b <= 1)
    if called is not None:
        ok &= called[:, 0::2] & called[:, 1::2]
    st = np.where(ok, np.where(a + b == 1, HET, HOM), MISS).astype(np.uint8)
    return st if samples is None else st[:, np.asarray(samples, dtype=np.int64)]


def qualifies(p, n_sites, length, n_het, n_missing):
    return (n_sites >= p["min_sites"] and length >= p["min_length"] and n_het <= p["max_het"] and n_missing <= p["max_missing"]
            and (p["max_bp_per_site"] == 0 or length <= p["max_bp_per_site"] * n_sites))


def scan(state, x, p):
    """The definition over a state table [K][n] and positions x [K] (None: x = k).  Returns a dict: the four tables and bin_runs / bin_length
    as uint64 arrays, `segments` = the qualifying runs as sorted tuples (sample, n_sites, n_het, n_missing, first, last), `runs` = EVERY
    maximal run as (sample, first, last, n_het, n_missing, length, qualifies), `in_run` [K][n] bool and `breaks` [K] bool."""
    state = np.asarray(state, dtype=np.uint8)
    K, n = state.shape
    W = p["window"]
    x = np.arange(K, dtype=np.int64) if x is None else np.asarray(x, dtype=np.int64)
    n_windows = K - W + 1 if K >= W else 0
    window_hom = np.zeros((max(n_windows, 0), n), dtype=bool)
    for t in range(n_windows):                              # rule 2, one window at a time
        rows = state[t:t + W]
        window_hom[t] = ((rows == HET).sum(axis=0) <= p["window_het"]) & ((rows == MISS).sum(axis=0) <= p["window_missing"])
    in_run = np.zeros((K, n), dtype=bool)
    for k in range(K if n_windows else 0):                  # rule 3
        lo, hi = max(0, k - W + 1), min(k, K - W)
        n_cov = hi - lo + 1
        n_hom = np.zeros(n, dtype=np.int64)
        for t in range(lo, hi + 1):
            n_hom += window_hom[t]
        in_run[k] = n_hom >= p["need"][n_cov]
    breaks = np.zeros(K, dtype=bool)
    for k in range(1, K):                                   # rule 5
        breaks[k] = p["max_gap"] > 0 and int(x[k]) - int(x[k - 1]) > p["max_gap"]
    edges = p["bin_edges"]
    nb = len(edges) + 1 if edges else 0
    out = {name: np.zeros(n, dtype=np.uint64) for name in TABLES}
    out["bin_runs"] = np.zeros((n, nb), dtype=np.uint64)
    out["bin_length"] = np.zeros((n, nb), dtype=np.uint64)
    segments, runs = [], []
    for i in range(n):
        k = 0
        while k < K:
            if not in_run[k, i]:
                k += 1
                continue
            first = k
            while k + 1 < K and in_run[k + 1, i] and not breaks[k + 1]:   # rule 6
                k += 1
            last = k
            k += 1
            n_sites = last - first + 1
            n_het = int((state[first:last + 1, i] == HET).sum())
            n_missing = int((state[first:last + 1, i] == MISS).sum())
            length = int(x[last]) - int(x[first]) + 1
            ok = qualifies(p, n_sites, length, n_het, n_missing)
            runs.append((i, first, last, n_het, n_missing, length, ok))
            if not ok:
                continue
            out["n_runs"][i] += 1
            out["sum_sites"][i] += n_sites
            out["sum_length"][i] += length
            out["longest_length"][i] = max(int(out["longest_length"][i]), length)
            if nb:
                b = sum(1 for e in edges if e <= length)
                out["bin_runs"][i, b] += 1
                out["bin_length"][i, b] += length
            segments.append((i, n_sites, n_het, n_missing, first, last))
    out.update(segments=sorted(segments, key=lambda s: (s[0], s[4])), runs=runs, in_run=in_run, breaks=breaks)
    return out


def segment_tuples(seg):
    """A structured segment array (ferromic_amd.device.ROH_SEGMENT_DTYPE) as the oracle's sorted tuples."""
    rows = [(int(s["sample"]), int(s["n_sites"]), int(s["n_het"]), int(s["n_missing"]), int(s["first_row"]), int(s["last_row"])) for s in seg]
    return sorted(rows, key=lambda s: (s[0], s[4]))


def checksum(result):
    """What ferromic_amd/csrc/roh_host_check.cpp prints for a scan: an order-free hash of the tables and segments."""
    mask = (1 << 64) - 1
    h = 0
    for name in TABLES:
        for i, v in enumerate(result[name].tolist()):
            h = (h + (int(v) + 1) * (0x9E3779B97F4A7C15 * (i + 1) & mask)) & mask
        h = (h * 31 + 7) & mask
    for s in result["segments"]:
        e = 0
        for v in s:
            e = (e * 1000003 + int(v) + 1) & mask
        h = (h + e * e) & mask
    return h


# ---- cohorts ----------------------------------------------------------------------------------------------------------------------------
def planted_states(K, n, seed, stretch=(20, 160), outside=(10, 120), het_in=0.02, het_out=0.4, miss=0.02):
    """[K][n] uint8 states: per sample alternating stretches inside (het rate het_in) and outside (het_out) a planted run, a few missing
    calls everywhere; sample 0 (when n > 2) is heterozygous nearly everywhere (no run) and the last sample starts and ends inside a run."""
    rng = np.random.default_rng(seed)
    st = np.zeros((K, n), dtype=np.uint8)
    for i in range(n):
        k, inside = 0, bool(rng.integers(2)) or i == n - 1
        while k < K:
            lo, hi = stretch if inside else outside
            length = int(rng.integers(lo, hi + 1))
            if i == n - 1 and k + length + hi >= K:
                length = K - k                               # the last sample's last stretch runs to the end
            rate = het_in if inside else het_out
            st[k:k + length, i] = (rng.random(min(length, K - k)) < rate).astype(np.uint8)
            k += length
            inside = not inside
        if i == n - 1 and K:
            st[max(0, K - stretch[0]):, i] = HOM
    if n > 2:
        st[:, 0] = (rng.random(K) < 0.6).astype(np.uint8)
    st[rng.random((K, n)) < miss] = MISS
    return st


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


def genotypes_from_states(st, seed, columns=None, high_allele=2, uncalled=True):
    """Alleles [K][2 S] uint8 and called [K][2 S] bool that realise the states: HOM as 0/0 or 1/1, HET as 0/1 or 1/0, MISS as an uncalled
    entry (one or both) or - half of the time, when high_allele > 1 - a called allele above 1 (always, with uncalled=False: the matrix
    has no called plane; called is then all True).  `columns` (S >= n) pads further samples with random genotypes."""
    assert uncalled or high_allele > 1 or not (st == MISS).any(), "a MISS needs an uncalled entry or an allele above 1"
    rng = np.random.default_rng(seed + 29)
    K, n = st.shape
    S = n if columns is None else columns
    a = rng.integers(0, 2, size=(K, S)).astype(np.uint8)
    b = rng.integers(0, 2, size=(K, S)).astype(np.uint8)
    full = np.zeros((K, S), dtype=np.uint8)
    full[:, :n] = st
    if S > n:
        full[:, n:] = rng.integers(0, 3 if (uncalled or high_allele > 1) else 2, size=(K, S - n))
    b = np.where(full == HOM, a, b)
    b = np.where(full == HET, 1 - a, b).astype(np.uint8)
    called_a = np.ones((K, S), dtype=bool)
    called_b = np.ones((K, S), dtype=bool)
    missing = full == MISS
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
