"""The admixture model without a device: the library's host twin (fmh_admix_step_host) against the long-double oracle of tests/admix_ref.py
within the derived bounds (tests/test_gpu_admix.py's docstring), the closed form at K = 1, the identity sum_k q_ik E_ik = 2 m_i, the tracks,
the default start and the extrapolation bit for bit against numpy restatements, Admixture.from_state, the argument refusals of the Python
surface, and the host arithmetic under ASan and UBSan (ferromic_amd/csrc/admix_host_check.cpp), whose checksum line is compared with the
library's own entry points over a splitmix64 cohort that tests/admix_ref.py restates."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import admix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.path.join(ROOT, "ferromic_amd", "bin")
SHAPES = [(65, 1030, 3), (40, 600, 2), (17, 257, 5), (1, 15, 1), (2, 64, 16), (16, 65, 9)]  # (samples, rows, K)


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm(dev):
    import ferromic

    return ferromic


def cohort(n, rows, K, seed=1):
    """A simulated cohort with edge rows: monomorphic, all missing, one called sample."""
    d, _, _ = R.simulate(n, rows, K, seed=seed + 31 * n + rows)
    d = d.copy()
    if rows > 6:
        d[0] = 0
        d[1] = 2
        d[2] = 3
        d[3] = 3
        d[3, 0] = 1
        d[4, :] = np.where(d[4] == 3, 3, 2)
    return d


def random_state(d, K, seed):
    rng = np.random.default_rng(seed)
    m = R.tracks(d)[4]
    q = rng.dirichlet(np.full(K, 0.7), size=d.shape[1]).clip(R.EPS, R.HI)
    q = q / q.sum(axis=1, keepdims=True)
    return q, rng.uniform(0.02, 0.98, size=(m, K))


@pytest.mark.parametrize("n,rows,K", SHAPES)
def test_twin_against_the_oracle(dev, n, rows, K):
    d = cohort(n, rows, K)
    q, f = random_state(d, K, seed=5)
    q1, f1, ll = dev.admix_step_host(d, q, f)
    rq, rf, rl, E = R.step(d, q, f)
    bf, bq, bl = R.bounds(d, K, rl)
    wf, wq, wl = R.worst(f1, rf, bf), R.worst(q1, rq, bq), abs(ll - rl) / (2 * bl) if bl else 0.0
    print(f"admix twin {n} x {rows}, K {K}: worst err / (2 bound): f {wf:.3e}, q {wq:.3e}, l {wl:.3e}")
    assert not np.isnan(q1).any() and not np.isnan(f1).any()
    assert wf <= 1.0 and wq <= 1.0 and wl <= 1.0
    # sum_k q_ik E_ik = 2 m_i, within the bound of E: (2 m + K + 8) u, and K + 2 more for the sum
    sites = R.tracks(d)[3].astype(np.float64)
    total = (q.astype(R.LD) * E).sum(axis=1)
    assert np.all(np.abs(total - 2 * sites) <= 2 * (2 * R.tracks(d)[4] + 2 * K + 10) * R.U * 2 * sites)


def test_tracks_equal_numpy(dev):
    for n, rows, K in SHAPES:
        d = cohort(n, rows, K, seed=3)
        got = dev.admix_tracks_host(d)
        usable, c, a, sites, m = R.tracks(d)
        assert np.array_equal(got.usable, usable) and np.array_equal(got.called, c) and np.array_equal(got.allele_count, a)
        assert np.array_equal(got.sample_sites, sites) and got.m == m
    assert (~R.tracks(cohort(17, 257, 5, seed=3))[0]).sum() >= 4


def test_one_component_is_the_closed_form(dev):
    d = cohort(23, 300, 1)
    usable, c, a, _, m = R.tracks(d)
    q, f = np.ones((23, 1)), np.full((m, 1), 0.3)
    q1, f1, _ = dev.admix_step_host(d, q, f)
    want = a[usable] / (2.0 * c[usable])
    assert np.all(q1 == 1.0)
    assert np.all(np.abs(f1[:, 0] - want) <= 8 * R.U * want)


def test_flags_leave_their_half_bit_identical(dev):
    d = cohort(17, 257, 5)
    q, f = random_state(d, 5, seed=8)
    both = dev.admix_step_host(d, q, f)
    only_q = dev.admix_step_host(d, q, f, update_f=False)
    only_f = dev.admix_step_host(d, q, f, update_q=False)
    neither = dev.admix_step_host(d, q, f, update_q=False, update_f=False, loglik=False)
    assert np.array_equal(only_q[1], f) and np.array_equal(only_q[0], both[0])
    assert np.array_equal(only_f[0], q) and np.array_equal(only_f[1], both[1])
    assert np.array_equal(neither[0], q) and np.array_equal(neither[1], f) and neither[2] is None
    assert only_q[2] == both[2] == only_f[2]


def test_no_usable_row_and_samples_without_sites(dev):
    d = np.full((5, 4), 3, dtype=np.uint8)
    d[1] = 0
    q = np.full((4, 2), 0.5)
    q1, f1, ll = dev.admix_step_host(d, q, np.zeros((0, 2)))
    assert np.array_equal(q1, q) and f1.shape == (0, 2) and ll == 0.0
    d = cohort(9, 40, 2)
    d[:, 3] = 3  # a sample that is never called keeps its row of Q
    q, f = random_state(d, 2, seed=1)
    q1, _, _ = dev.admix_step_host(d, q, f)
    assert np.array_equal(q1[3], q[3]) and not np.array_equal(q1[2], q[2])


def test_start_is_the_numpy_restatement(dev):
    for n, rows, K, seed in [(7, 40, 3, 0), (1, 9, 1, 5), (20, 65, 16, 2 ** 63 + 11)]:
        usable, c, a, _, m = R.tracks(cohort(n, rows, K))
        q, f = dev.admix_start(c[usable], a[usable], n, K, seed)
        rq, rf = R.start(c[usable], a[usable], n, K, seed)
        assert np.array_equal(q.view(np.uint64), rq.view(np.uint64)) and np.array_equal(f.view(np.uint64), rf.view(np.uint64))
        assert np.all(np.abs(q.sum(axis=1) - 1.0) < 1e-14) and f.min() >= 0.01 and f.max() <= 0.99
    with pytest.raises(RuntimeError):
        dev.admix_start(np.array([4]), np.array([0]), 3, 2)  # a row that is not usable


def test_accelerate_is_the_numpy_restatement(dev):
    rng = np.random.default_rng(4)
    n, m, K = 9, 31, 3
    s0 = (rng.dirichlet(np.ones(K), size=n), rng.uniform(0.05, 0.95, size=(m, K)))
    s1 = (s0[0] + 0.01 * rng.normal(size=(n, K)), s0[1] + 0.01 * rng.normal(size=(m, K)))
    curved = (s1[0] + 0.9 * (s1[0] - s0[0]) + 1e-5 * rng.normal(size=(n, K)), s1[1] + 0.9 * (s1[1] - s0[1]))  # slow geometric convergence: alpha near 10
    far = (s1[0] + 3 * (s1[0] - s0[0]) + 1e-3, s1[1] + 3 * (s1[1] - s0[1]))  # v larger than r: alpha clipped to 1
    seen = set()
    for s2 in (curved, far):
        qa, fa, alpha = dev.admix_accelerate(s0, s1, s2)
        rq, rf, ralpha = R.accelerate(s0, s1, s2)
        assert alpha == ralpha and np.array_equal(qa.view(np.uint64), rq.view(np.uint64)) and np.array_equal(fa.view(np.uint64), rf.view(np.uint64))
        assert fa.min() >= R.EPS and fa.max() <= R.HI and np.all(np.abs(qa.sum(axis=1) - 1.0) < 1e-14)
        seen.add(alpha == 1.0)
    assert seen == {True, False}, "alpha clipped to 1 and alpha above 1 both occur"
    # sum v^2 = 0: the third state, alpha = 0
    same = (s0[0].copy(), s0[1].copy())
    qa, fa, alpha = dev.admix_accelerate(same, same, same)
    assert alpha == 0.0 and np.array_equal(qa, same[0]) and np.array_equal(fa, same[1])
    assert R.accelerate(same, same, same)[2] == 0.0


def test_from_state(fm):
    q = np.array([[0.25, 0.75], [0.5, 0.5], [1.0 - 1e-5, 1e-5]])
    f = np.array([[0.1, 0.9], [np.nan, np.nan], [0.3, 0.4], [0.5, 0.5]])
    a = fm.Admixture.from_state(q, f, called=[3, 0, 3, 2], allele_count=[2, 0, 3, 1], sample_sites=[3, 3, 2], positions=[5, 9, 11, 20],
                                log_likelihood=-12.5, trace=[-14.0, -13.0], steps=2, cycles=1, accepted=0, converged=True)
    assert a.k == 2 and np.array_equal(a.q, q) and np.array_equal(a.frequencies, f, equal_nan=True)
    assert np.array_equal(a.usable, [True, False, True, True]) and a.n_usable == 3
    assert np.array_equal(a.called, [3, 0, 3, 2]) and np.array_equal(a.allele_count, [2, 0, 3, 1]) and np.array_equal(a.sample_sites, [3, 3, 2])
    assert np.array_equal(a.samples, [0, 1, 2]) and np.array_equal(a.sites, [0, 1, 2, 3]) and np.array_equal(a.positions, [5, 9, 11, 20])
    assert a.log_likelihood == -12.5 and np.array_equal(a.trace, [-14.0, -13.0]) and (a.steps, a.cycles, a.accepted, a.converged) == (2, 1, 0, True)
    assert "k=2" in repr(a)
    with pytest.raises(ValueError, match="q must"):
        fm.Admixture.from_state(np.zeros(3), f)
    with pytest.raises(ValueError, match="frequencies must"):
        fm.Admixture.from_state(q, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="k must"):
        fm.Admixture.from_state(np.zeros((2, 17)), np.zeros((4, 17)))
    with pytest.raises(ValueError, match="called has"):
        fm.Admixture.from_state(q, f, called=[1, 2])
    with pytest.raises(ValueError, match="usable must"):
        fm.Admixture.from_state(q, f, usable=[True])


def records(K=6, n=4):
    return [{"position": 10 * k + 1, "genotypes": [(k % 2, (k + s) % 2) for s in range(n)]} for k in range(K)]


def test_python_refusals(fm):
    assert fm.Admixture.__module__.endswith("_core") and callable(fm.admixture) and hasattr(fm.Population, "admixture")
    V = records()
    good_q = np.full((4, 2), 0.5)
    for kwargs, match in [
        (dict(k=0), "k must"), (dict(k=17), "k must"), (dict(k=2, tol=-1.0), "tol"), (dict(k=2, tol=float("nan")), "tol"),
        (dict(k=2, max_steps=-1), "max_steps"), (dict(k=2, seed=-3), "seed"), (dict(k=2, samples=[0, 9]), "outside"),
        (dict(k=2, samples=[2, 1]), "ascending"), (dict(k=2, samples=[]), "at least one sample"), (dict(k=2, init=5), "init must"),
        (dict(k=2, init=(good_q,)), "init must"), (dict(k=2, init=(np.full((3, 2), 0.5), np.full((6, 2), 0.5))), "init's Q"),
        (dict(k=2, init=(np.full((4, 3), 0.3), np.full((6, 3), 0.5))), "init's Q"), (dict(k=2, init=(np.zeros((4, 2)), np.full((6, 2), 0.5))), "outside"),
        (dict(k=2, init=(good_q, np.full((6, 3), 0.5))), "init's F"), (dict(k=2, init=(good_q, None)), "init's F is None"),
        (dict(k=2, init=(good_q, np.full((6, 2), 0.5)), frequencies=np.full((6, 2), 0.5)), "both given"),
        (dict(k=2, frequencies=np.full((6, 3), 0.5)), "frequencies must"), (dict(k=2, frequencies=np.full(6, 0.5)), "frequencies must"),
    ]:
        with pytest.raises(ValueError, match=match):
            fm.admixture(V, **kwargs)
    with pytest.raises(TypeError):
        fm.admixture(V, 2, samples=["a"])
    with pytest.raises(ValueError, match="ploidy"):
        fm.admixture([{"position": 1, "genotypes": [(0,), (1,)]}], 2)
    pop = fm.Population("p", V, [(0, 0), (0, 1), (1, 0), (1, 1)], 100)
    with pytest.raises(ValueError, match="k must"):
        pop.admixture(0)


def test_c_abi_refusals_without_a_device(dev):
    from ferromic_amd import _abi as abi

    lib = abi.load()
    d = np.zeros((3, 2), dtype=np.uint8)
    q, f = np.full((2, 2), 0.5), np.full((0, 2), 0.5)
    out = np.zeros((2, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    invalid = [
        lib.fmh_admix_step_host(p(d), 3, 0, 2, p(q), p(f), p(out), p(f), None, 3, None),
        lib.fmh_admix_step_host(None, 3, 2, 2, p(q), p(f), p(out), p(f), None, 3, None),
        lib.fmh_admix_step_host(p(d), 3, 2, 0, p(q), p(f), p(out), p(out), None, 3, None),
        lib.fmh_admix_step_host(p(d), 3, 2, 17, p(q), p(f), p(out), p(out), None, 3, None),
        lib.fmh_admix_step_host(p(d), 3, 2, 2, p(q), p(f), p(q), p(out), None, 3, None),
        lib.fmh_admix_step_host(p(d), 3, 2, 2, p(q), p(f), None, p(out), None, 3, None),
        lib.fmh_admix_step_host(p(d), 3, 2, 2, p(q), p(f), p(out), p(d), None, 4, None),
        lib.fmh_admix_start(None, None, 0, 2, 0, 0, p(q), None),
        lib.fmh_admix_start(None, None, 0, 2, 2, 0, None, None),
        lib.fmh_admix_accelerate(p(q), None, p(q), None, p(q), None, 2, 0, 2, p(out), None, None),
        lib.fmh_admix_accelerate(p(q), None, p(q), None, p(q), None, 2, 0, 99, p(out), None, C.byref(C.c_double())),
        lib.fmh_admix_create(None, None, 1, 0, 0, None, C.byref(C.c_void_p()), None),
        lib.fmh_admix_info(None, None),
        lib.fmh_admix_step(None, 2, p(q), p(f), p(out), p(f), None, 3, None),
    ]
    assert invalid == [abi.FMH_ERR_INVALID] * len(invalid), invalid
    lib.fmh_admix_destroy(None)
    for key, default in (("FMH_ADMIX_ITEM_ROWS", 0), ("FMH_ADMIX_BUDGET_BYTES", 4 << 30)):
        value = C.c_longlong(-1)
        assert lib.fmh_get_option(key.encode(), C.byref(value)) == 0 and value.value == default


def test_host_arithmetic_under_sanitizers(dev):
    program = os.path.join(BIN_DIR, "admix_host_check.asan")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    usable_total = 0
    for seed, rows, n, K in [(1, 90, 7, 3), (2, 65, 9, 1), (3, 120, 5, 16), (4, 1, 3, 2)]:
        res = subprocess.run([program, str(seed), str(rows), str(n), str(K)], capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        d, start_seed = R.check_cohort(seed, rows, n)
        usable, c, a, _, m = R.tracks(d)
        s0 = dev.admix_start(c[usable], a[usable], n, K, start_seed)
        q1, f1, ll = dev.admix_step_host(d, *s0)
        q2, f2, _ = dev.admix_step_host(d, q1, f1, loglik=False)
        qa, fa, alpha = dev.admix_accelerate(s0, (q1, f1), (q2, f2))
        q4, f4, _ = dev.admix_step_host(d, qa, fa, loglik=False, update_f=False)
        h, m = R.checksum(d, [s0, (q1, f1), (q2, f2), (qa, fa), (q4, f4)], alpha)
        usable_total += m
        lines = res.stdout.splitlines()
        assert lines[0] == "admix_host_check: %d rows x %d samples, K %d, %d usable, checksum %016x" % (rows, n, K, m, h), (lines, h)
        assert lines[1].split()[0] == "loglik" and abs(float(lines[1].split()[1]) - ll) <= 1e-9 * max(1.0, abs(ll)) and float(lines[1].split()[3]) == alpha
    assert usable_total > 150
