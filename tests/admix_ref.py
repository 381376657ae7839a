"""The admixture model's oracle, written from the definition in include/ferromic_hip.h: one EM step in np.longdouble, rounded once; the
tracks; numpy restatements of the default start and of the SQUAREM extrapolation in the stated order; the derived error bounds; a plain
and an accelerated fit; a simulated cohort; and the checksum of ferromic_amd/csrc/admix_host_check.cpp.

A dosage table is [rows][n] uint8: 0, 1, 2, or 3 = not called (tests/grm_ref.py: codes)."""

import numpy as np

from tests import grm_ref

LD = np.longdouble
U = 2.0 ** -53
EPS = 1e-5
HI = 1.0 - 1e-5  # the f64 value the code clamps to
MASK64 = (1 << 64) - 1


def tracks(d):
    """(usable bool [rows], c, a uint32 [rows], sample_sites uint64 [n], m)."""
    called = d <= 2
    c = called.sum(axis=1).astype(np.uint32)
    a = np.where(called, d, 0).sum(axis=1).astype(np.uint32)
    usable = (c > 0) & (a > 0) & (a.astype(np.int64) < 2 * c.astype(np.int64))
    sites = called[usable].sum(axis=0).astype(np.uint64)
    return usable, c, a, sites, int(usable.sum())


def step(d, q, f, update_q=True, update_f=True, swap_hom=False, missing_as_ref=False, swap_uv=False, g_is_f=False, transpose_q=False, LD=LD):
    """(q', f', l, E) of one EM step in np.longdouble, q', f', l rounded once to f64 (E stays long double).  f is [m][K] over the usable rows.
    The keyword faults are what a confused kernel would compute; the tracks stay the true ones.  LD=np.float64: the same formulas in plain
    numpy f64 (the long fits, where the oracle's precision is not the point)."""
    usable, _, _, sites, m = tracks(d)
    du = d[usable]
    if swap_hom:
        du = np.where(du == 0, 2, np.where(du == 2, 0, du)).astype(np.uint8)
    cal = du <= 2
    if missing_as_ref:
        du = np.where(cal, du, 0).astype(np.uint8)
        cal = np.ones_like(cal)
    g = np.where(cal, du, 0).astype(LD)
    Q, F = np.asarray(q, dtype=np.float64).astype(LD), np.asarray(f, dtype=np.float64).astype(LD)
    if transpose_q:
        Q = Q.T.copy()
    G = F if g_is_f else (1.0 - np.asarray(f, dtype=np.float64)).astype(LD)  # G = fl(1 - F)
    h0, h1 = F @ Q.T, G @ Q.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(cal, g / h0, LD(0))
        v = np.where(cal, (2 - g) / h1, LD(0))
        if swap_uv:
            u, v = v, u
        ll = np.where(cal, g * np.log(h0) + (2 - g) * np.log(h1), LD(0)).sum()
    A, B = u @ Q, v @ Q
    E = u.T @ F + v.T @ G
    f_new = F
    if update_f:
        fa, gb = F * A, G * B
        f_new = np.clip(fa / (fa + gb), LD(EPS), LD(HI))
    q_new = np.asarray(q, dtype=np.float64).astype(LD).copy()
    if update_q:
        live = sites > 0
        q0 = np.clip(q_new[live] * E[live] / (2 * sites[live].astype(LD))[:, None], LD(EPS), LD(HI))
        q_new[live] = q0 / q0.sum(axis=1, keepdims=True)
    return q_new.astype(np.float64), f_new.astype(np.float64), float(ll), E


def gamma(d):
    usable, _, _, sites, _ = tracks(d)
    return int(sites.sum())


def bounds(d, K, ll):
    """(relative bound of f', relative bound of q', absolute bound of l): the derivation is in tests/test_gpu_admix.py's docstring."""
    _, _, _, _, m = tracks(d)
    n = d.shape[1]
    big = gamma(d)
    return 2 * (n + K + 16) * U, 2 * (2 * m + 2 * K + 24) * U, 2 * big * (K + 40) * U + (2 * big + 2) * U * abs(ll)


def worst(got, ref, rel):
    """max |got - ref| / (2 rel |ref|): at most one inside twice the bound."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.size == 0:
        return 0.0
    return float((np.abs(got.astype(LD) - ref.astype(LD)) / (2 * rel * np.abs(ref).astype(LD))).max())


# ---- the default start and the extrapolation, restated ---------------------------------------------------------------------------------------
def mix(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def unit(seed_mixed, t):
    return float(mix((seed_mixed + t) & MASK64) >> 11) * 2.0 ** -53


def start(c, a, n, K, seed):
    s = mix(seed)
    q = np.empty((n, K))
    for i in range(n):
        w = [1.0 + unit(s, i * K + k) for k in range(K)]
        total = 0.0
        for x in w:
            total += x
        q[i] = [x / total for x in w]
    f = np.empty((len(c), K))
    for j in range(len(c)):
        p = float(a[j]) / (2.0 * float(c[j]))
        for k in range(K):
            f[j, k] = min(max(p + 0.2 * (unit(s, (1 << 40) + j * K + k) - 0.5), 0.01), 0.99)
    return q, f


def renormalise(q):
    out = np.clip(q, EPS, HI)
    for i in range(out.shape[0]):
        total = 0.0
        for k in range(out.shape[1]):
            total += out[i, k]
        out[i] = out[i] / total
    return out


def accelerate(s0, s1, s2):
    """(qa, fa, alpha) in the stated order: the sums over Q then F, ascending index, plain f64."""
    (q0, f0), (q1, f1), (q2, f2) = s0, s1, s2
    sr = sv = 0.0
    for x0, x1, x2 in ((q0, q1, q2), (f0, f1, f2)):
        r = (x1 - x0).ravel()
        v = ((x2 - x1) - (x1 - x0)).ravel()
        for e in range(r.size):
            sr += r[e] * r[e]
            sv += v[e] * v[e]
    if sv == 0.0:
        return q2.copy(), f2.copy(), 0.0
    alpha = max(1.0, float(np.sqrt(np.float64(sr) / np.float64(sv))))

    def move(x0, x1, x2):
        r = x1 - x0
        v = (x2 - x1) - r
        return (x0 + (2.0 * alpha) * r) + (alpha * alpha) * v

    return renormalise(move(q0, q1, q2)), np.clip(move(f0, f1, f2), EPS, HI), alpha


# ---- fits by the oracle's own step -------------------------------------------------------------------------------------------------------------
def fit_plain(d, q, f, steps):
    trace = []
    for _ in range(steps):
        q, f, ll, _ = step(d, q, f, LD=np.float64)
        trace.append(ll)
    return q, f, trace


def fit_cycles(d, q, f, cycles):
    """(q, f, l0 of every cycle, accepted)."""
    l0s, accepted = [], 0
    for _ in range(cycles):
        q1, f1, l0, _ = step(d, q, f, LD=np.float64)
        q2, f2, l1, _ = step(d, q1, f1, LD=np.float64)
        l0s.append(l0)
        qa, fa, alpha = accelerate((q, f), (q1, f1), (q2, f2))
        if alpha == 0.0:
            q, f = q2, f2
            continue
        q3, f3, la, _ = step(d, qa, fa, LD=np.float64)
        if np.isfinite(la) and la >= l1:
            q, f, accepted = q3, f3, accepted + 1
        else:
            q, f = q2, f2
    return q, f, l0s, accepted


def simulate(n, rows, K, seed, missing=0.02):
    """(dosage table, Q, F [rows][K]): Q ~ Dirichlet(0.3), F = clip(ancestral + N(0, 0.25), 0.02, 0.98), binomial genotypes."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.full(K, 0.3), size=n)
    ancestral = rng.uniform(0.05, 0.95, size=(rows, 1))
    F = np.clip(ancestral + rng.normal(0.0, 0.25, size=(rows, K)), 0.02, 0.98)
    p = F @ Q.T
    d = rng.binomial(2, p).astype(np.uint8)
    d[rng.random(d.shape) < missing] = 3
    return d, np.clip(Q, EPS, HI), F


# ---- the seeded cohort of ferromic_amd/csrc/admix_host_check.cpp, and its checksum ---------------------------------------------------------
def check_cohort(seed, rows, n):
    """(dosage, the generator's state after it: the seed of the program's default start)."""
    r = grm_ref.SplitMix64(seed)
    d = np.zeros((rows, n), dtype=np.uint8)
    for k in range(rows):
        t, gaps = r.next() % 17, r.next() % 32
        for s in range(n):
            g = int(r.next() % 16 < t) + int(r.next() % 16 < t)
            if gaps == 0 or (gaps < 4 and r.next() % 4 == 0):
                g = 3
            d[k, s] = g
    return d, r.state


def checksum(d, states, alpha):
    """The checksum line's number for the five states [(q, f)] the program walks through."""
    usable, c, a, sites, m = tracks(d)
    h = m * 1000003 + grm_ref.bits_of(alpha)
    for r in range(d.shape[0]):
        h += (int(usable[r]) + 1) * (0x9E3779B97F4A7C15 * (r + 1)) + int(c[r]) * (2 * r + 1) + int(a[r]) * (2 * r + 3)
    for i in range(d.shape[1]):
        h += int(sites[i]) * (0xBF58476D1CE4E5B9 + i)
    for s, (q, f) in enumerate(states):
        for e, v in enumerate(np.asarray(q).ravel()):
            h += grm_ref.bits_of(v) * (2 * e + 5 + 2 * s)
        for e, v in enumerate(np.asarray(f).ravel()):
            h += grm_ref.bits_of(v) * (2 * e + 7 + 2 * s)
    return h & MASK64, m
