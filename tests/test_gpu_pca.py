"""Haplotype PCA on the device against tests/pca_ref.py (the numpy restatement of src/pca.rs).

Gram: entry by entry against Z Z^T / (n - 1), with a DERIVED tolerance - any summation order of m f64 products is within
(m + 2) * 2^-53 * sum_k |z_ik| |z_jk| / (n - 1) of the exact value (m - 1 additions, one product rounding, the division), numpy's own sum
has the same bound, so twice that separates the two.  One dropped, doubled or mis-weighted site moves an entry by about 1 / (n - 1),
five to nine orders above the bound.

Scores: the CPU answer is computed twice (Gram + eigh restatement, and thin SVD); their largest disagreement d0 measures what a different
summation order does to these eigenvectors (rounding error over the spectral gap); the device must be within 32 * d0 of the
restatement.  Before the device result is looked at the test checks that the CPU pair is conclusive: 32 * d0 <= 1e-8 * max |coordinate|
and every requested component's relative gap (lambda_k - lambda_k+1) / lambda_1 >= 1e-5.
"""

import os

import numpy as np
import pytest

from tests import pca_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm():
    import ferromic

    return ferromic


def binary_rows(rng, rows, n):
    """rows x n 0/1 uint8 with both alleles present in every row (a positive variance)."""
    freq = rng.uniform(0.08, 0.92, size=(rows, 1))
    x = (rng.random((rows, n)) < freq).astype(np.uint8)
    x[:, 0] = 1
    x[:, n - 1] = 0
    return x


def gram_expectation(x_kept, n):
    hi, lo = R.set_clear_values(x_kept.sum(axis=1), n)
    z = np.where(x_kept.T == 1, hi[None, :], lo[None, :])  # n x m, the very operands the device expands
    m = x_kept.shape[0]
    expected = z @ z.T / float(n - 1)
    bound = 2.0 * (m + 2) * EPS * (np.abs(z) @ np.abs(z).T) / float(n - 1)
    return hi, lo, z, expected, bound


def check_gram(dev, fmh_opts, n, m, layout, splits, seed):
    rng = np.random.default_rng(seed)
    rows = m + m // 3 + 7
    x = binary_rows(rng, rows, n)
    # kept rows: a sorted subset that does not start at row 0 and has holes
    kept = np.sort(rng.choice(np.arange(3, rows), size=m, replace=False)).astype(np.uint64)
    if layout == "bytes":
        fmh_opts.setenv("FMH_LAYOUT", "bytes")
    if splits:
        fmh_opts.setenv("FMH_PCA_SPLITS", splits)
    dm = dev.DeviceMatrix.from_host(x, None, rows, n // 2, 2, 1)
    try:
        hi, lo, _, expected, bound = gram_expectation(x[kept.astype(np.int64)], n)
        got = dev.pca_gram(dm, kept, hi, lo)
        again = dev.pca_gram(dm, kept, hi, lo)
    finally:
        dm.close()
    err = np.abs(got - expected)
    worst = float((err / bound).max())
    print(f"gram n={n} m={m} layout={layout} splits={splits}: max err {err.max():.3e}, max err/bound {worst:.3e}")
    assert np.all(err <= bound), (n, m, layout, splits, worst)
    assert np.array_equal(got, got.T), "the Gram must be exactly symmetric"
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "two runs on the same input must give the same bits"


GRAM_CASES = [
    # n, m_kept, layout, FMH_PCA_SPLITS (0 = the library's choice)
    (2, 1, "packed", 0),
    (6, 63, "packed", 0),
    (6, 1, "bytes", 0),
    (96, 65, "bytes", 0),
    (96, 4097, "packed", 5),
    (130, 4097, "packed", 0),
    (130, 4097, "packed", 1),
    (130, 63, "packed", 0),
    (512, 4097, "bytes", 3),
    (512, 65, "packed", 1),
    (1002, 4097, "packed", 0),
    (1002, 4097, "bytes", 1),
    (1002, 1, "packed", 0),
]


@pytest.mark.parametrize("n,m,layout,splits", GRAM_CASES)
def test_gram_entry_by_entry(dev, fmh_opts, n, m, layout, splits):
    check_gram(dev, fmh_opts, n, m, layout, splits, seed=1000 * n + m)


def test_scan_sites_flags_and_counts(dev, fmh_opts):
    """(The per-row tables, rows wider than 4 096 columns, every upload route and row ranges: tests/test_gpu_pca_scan.py.)"""
    rng = np.random.default_rng(5)
    rows, n = 300, 70
    x = binary_rows(rng, rows, n)
    missing = np.zeros((rows, n), dtype=bool)
    x[10, 3] = 2
    x[11, 69] = 3
    missing[20, 0] = True
    missing[21, 69] = True
    missing[22, 33] = True
    x[22, 34] = 2
    x[23, 5] = 2
    missing[23, 5] = True  # an allele above 1 that is not called does not count
    words = np.zeros((rows * n + 63) // 64, dtype=np.uint64)
    for r, c in zip(*np.nonzero(missing)):
        i = int(r) * n + int(c)
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    exp_flags = np.where(missing.any(axis=1), dev.PCA_SITE_UNCALLED, 0) | np.where(((x > 1) & ~missing).any(axis=1), dev.PCA_SITE_HIGH_ALLELE, 0)
    exp_alt = ((x == 1) & ~missing).sum(axis=1)
    for layout in ("packed", "bytes"):
        fmh_opts.setenv("FMH_LAYOUT", layout)
        dm = dev.DeviceMatrix.from_host(x, words, rows, n // 2, 2, 3)
        try:
            alt, flags = dev.pca_scan_sites(dm)
            alt2, flags2 = dev.pca_scan_sites(dm, 7, 100)
        finally:
            dm.close()
        assert np.array_equal(flags, exp_flags.astype(np.uint8)), layout
        assert np.array_equal(alt, exp_alt.astype(np.uint32)), layout
        assert np.array_equal(alt2, alt[7:107]) and np.array_equal(flags2, flags[7:107])


def test_gram_argument_errors(dev):
    from ferromic_amd import _abi

    x = np.zeros((4, 6), dtype=np.uint8)
    dm = dev.DeviceMatrix.from_host(x, None, 4, 2, 3, 1)  # ploidy 3
    with pytest.raises(_abi.FerromicHipError, match="ploidy"):
        dev.pca_gram(dm, [0], [1.0], [0.0])
    dm.close()
    dm = dev.DeviceMatrix.from_host(x, None, 4, 3, 2, 1)
    with pytest.raises(_abi.FerromicHipError, match="n_kept"):
        dev.pca_gram(dm, [], [], [])
    with pytest.raises(_abi.FerromicHipError, match="exceeds"):
        dev.pca_gram(dm, [4], [1.0], [0.0])
    dm.close()


def cpu_pair(genotypes, n_components):
    """(restatement scores with canonical signs, eigenvalues, d0) - and the check that this CPU pair is conclusive."""
    kept, complete = R.site_filter(genotypes)
    x = R.haplotype_matrix(genotypes, kept)
    k = R.clamp_components(n_components, complete, x.shape[0])
    a, w = R.transform(x, k)
    a = R.canonical_signs(a)
    b = R.canonical_signs(R.transform_svd(x, k))
    d0 = float(np.abs(a - b).max())
    assert 32 * d0 <= 1e-8 * np.abs(a).max(), ("CPU pair inconclusive", d0)
    gaps = (w[:k] - w[1:k + 1]) / w[0]
    assert gaps.min() >= 1e-5, ("spectral gap too small for this seed", gaps)
    return a, w, d0, kept


def check_scores(got, a, w, d0, n, what):
    got = R.canonical_signs(got)
    assert got.shape == a.shape
    err = float(np.abs(got - a).max())
    print(f"{what}: score err {err:.3e}, 32*d0 {32 * d0:.3e}, within 1.28e-10: {err <= 1.28e-10}")
    assert err <= 32 * d0, (what, err, d0)
    k = a.shape[1]
    # gap-free: a column's variance is its eigenvalue (an eigenvalue is backward stable whatever the gap); columns are orthogonal
    # (a symmetric solver's vectors lose orthogonality at the order of n eps; a modest constant, 1000 here)
    var = (got ** 2).sum(axis=0) / float(n - 1)
    assert np.all(np.abs(var - w[:k]) <= 1e-11 * w[:k]), (what, var, w[:k])
    norm = np.sqrt((got ** 2).sum(axis=0))
    cos = (got.T @ got) / np.outer(norm, norm)
    off = np.abs(cos - np.diag(np.diag(cos))).max() if k > 1 else 0.0
    assert off <= 1000 * n * EPS, (what, off)


PYBENCH_SHAPES = [(512, 48), (4096, 96), (16384, 128), (65536, 256)]  # the reference's PCA benchmark suite, 6 components


@pytest.mark.parametrize("variants,samples", PYBENCH_SHAPES)
def test_scores_pybench_cohorts(fm, variants, samples):
    g = R.pybench_cohort(variants, samples, seed=variants + samples)
    a, w, d0, kept = cpu_pair(g, 6)
    positions = np.arange(variants, dtype=np.int64) * 7 + 11
    names = [f"sample_{i}" for i in range(samples)]
    res = fm.chromosome_pca({"genotypes": g, "positions": positions}, names, 6)
    assert res.haplotype_labels == [f"sample_{i}_{s}" for i in range(samples) for s in "LR"]
    assert np.array_equal(res.positions, positions[kept]) and res.positions.dtype == np.int64
    assert res.coordinates.flags["C_CONTIGUOUS"] and res.coordinates.dtype == np.float64
    assert repr(res) == f"ChromosomePcaResult(haplotypes={2 * samples}, components=6, variants={kept.size})"
    check_scores(res.coordinates, a, w, d0, 2 * samples, f"pybench {variants}x{samples}")


def test_scores_four_populations(fm):
    g = R.pybench_cohort(6000, 120, seed=44, scale=0.1, populations=4)
    a, w, d0, _ = cpu_pair(g, 3)
    res = fm.chromosome_pca({"genotypes": g, "positions": np.arange(6000, dtype=np.int64)}, [f"s{i}" for i in range(120)], 3)
    check_scores(res.coordinates, a, w, d0, 240, "four populations")


def test_trace_of_all_eigenvalues(dev):
    """sum of ALL eigenvalues = trace of the Gram = the number of kept sites (every standardised column has variance 1)."""
    g = R.pybench_cohort(512, 48, seed=560)
    kept, _ = R.site_filter(g)
    flat = g.reshape(512, 96).astype(np.uint8)
    hi, lo = R.set_clear_values(flat[kept].sum(axis=1), 96)
    dm = dev.DeviceMatrix.from_host(flat, None, 512, 48, 2, 1)
    try:
        buf = dev.pca_gram_device(dm, kept, hi, lo)
        values, scores = dev.pca_eigen_scores(dm.device, buf, 96)
    finally:
        dm.close()
    assert np.all(np.diff(values) <= 0)
    # n eigenvalues, each within n eps lambda_1 of exact: n^2 eps ~ 1e-12 relative
    assert abs(values.sum() - kept.size) <= 1e-11 * kept.size, (values.sum(), kept.size)
    assert scores.shape == (96, 96)


def test_host_and_rocsolver_eigen_agree(fm, fmh_opts):
    from ferromic_amd import _abi

    for variants, samples in PYBENCH_SHAPES[:2]:
        g = R.pybench_cohort(variants, samples, seed=variants + samples)
        a, w, d0, _ = cpu_pair(g, 6)
        arg = {"genotypes": g, "positions": np.arange(variants, dtype=np.int64)}
        names = [f"s{i}" for i in range(samples)]
        fmh_opts.setenv("FMH_PCA_EIGEN", "host")
        host = fm.chromosome_pca(arg, names, 6).coordinates
        check_scores(host, a, w, d0, 2 * samples, f"host solver {variants}x{samples}")
        fmh_opts.setenv("FMH_PCA_EIGEN", "rocsolver")
        try:
            solver = fm.chromosome_pca(arg, names, 6).coordinates
        except RuntimeError as e:
            if "rocSOLVER is not available" in str(e):  # the library cannot be loaded here; anything else is a defect
                pytest.skip(f"rocSOLVER cannot be loaded on this machine: {e}")
            raise
        check_scores(solver, a, w, d0, 2 * samples, f"rocSOLVER {variants}x{samples}")
        assert np.abs(R.canonical_signs(host) - R.canonical_signs(solver)).max() <= 64 * d0  # both within 32 d0 of the restatement
        assert _abi.get_option("FMH_PCA_EIGEN") == 2


def sprinkled_cohort():
    g = R.pybench_cohort(900, 40, seed=91).astype(np.int16)
    rng = np.random.default_rng(92)
    for r in rng.choice(900, size=60, replace=False):
        g[r, rng.integers(40), rng.integers(2)] = -1
    for r in rng.choice(900, size=50, replace=False):
        g[r, rng.integers(40), rng.integers(2)] = rng.integers(2, 300)
    return g


def test_api_inputs_filter_and_labels(fm):
    g = sprinkled_cohort()
    positions = np.cumsum(np.arange(1, 901, dtype=np.int64))
    names = [f"n{i}" for i in range(40)]
    labels, exp, exp_pos = R.chromosome_pca(g, positions, names, 5)
    a, w, d0, _ = cpu_pair(g, 5)
    # dict input
    res = fm.chromosome_pca({"genotypes": g, "positions": positions}, names, 5)
    assert res.haplotype_labels == labels and np.array_equal(res.positions, exp_pos)
    check_scores(res.coordinates, a, w, d0, 80, "dict input")
    # non-contiguous genotypes: every second row / sample of a larger array
    big = np.full((1800, 80, 2), 7, dtype=np.int16)
    big[::2, ::2, :] = g
    view = big[::2, ::2, :]
    assert not view.flags["C_CONTIGUOUS"]
    res2 = fm.chromosome_pca({"genotypes": view, "positions": positions}, names, 5)
    assert np.array_equal(res2.positions, exp_pos) and np.array_equal(res2.coordinates, res.coordinates)
    # list of (position, genotypes) tuples with list genotypes: None = missing, a scalar a = (a, a)
    records = []
    for r in range(900):
        calls = []
        for s in range(40):
            left, right = int(g[r, s, 0]), int(g[r, s, 1])
            if left < 0 or right < 0:
                calls.append(None)
            elif left == right and s % 3 == 0:
                calls.append(left)
            else:
                calls.append([left, right] if s % 2 else (left, right))
        records.append((int(positions[r]), calls))
    g_list = g.copy()
    g_list[(g < 0).any(axis=2)] = -1  # None makes the whole call missing
    _, _, exp_pos_l = R.chromosome_pca(g_list, positions, names, 5)
    a_l, w_l, d0_l, _ = cpu_pair(g_list, 5)
    res3 = fm.chromosome_pca(records, names, 5)
    assert np.array_equal(res3.positions, exp_pos_l)
    check_scores(res3.coordinates, a_l, w_l, d0_l, 80, "list input")


def test_api_component_clamps_and_errors(fm):
    names = [f"n{i}" for i in range(5)]
    g = R.pybench_cohort(200, 5, seed=3)
    positions = np.arange(200, dtype=np.int64)
    kept, complete = R.site_filter(g)
    # more components than min(m, n): the width is min(n_components, min(m, n))
    res = fm.chromosome_pca({"genotypes": g, "positions": positions}, names, 50)
    assert res.coordinates.shape == (10, min(50, complete, 10, kept.size))
    # m_kept <= n: seven kept sites, ten haplotypes
    few = g[kept[:7]]
    res = fm.chromosome_pca({"genotypes": few, "positions": positions[:7]}, names, 3)
    assert res.coordinates.shape == (10, 3)
    a, w, d0, _ = cpu_pair(few, 3)
    check_scores(res.coordinates, a, w, d0, 10, "seven sites, ten haplotypes")
    # three complete sites of which two carry an allele 2: dense input counts one complete site, Variant input (tuple genotypes are
    # not the dense list form) three; the kept sites are a subset of the complete ones under both rules, so the width is the same
    tri = g[kept[:3]].astype(np.int16)
    tri[1, 0, 0] = 2
    tri[2, 1, 1] = 2
    dense = fm.chromosome_pca({"genotypes": tri, "positions": positions[:3]}, names, 3)
    assert dense.coordinates.shape == (10, 1) and np.array_equal(dense.positions, positions[:1])
    as_variants = [(int(positions[r]), tuple((int(tri[r, s, 0]), int(tri[r, s, 1])) for s in range(5))) for r in range(3)]
    sparse = fm.chromosome_pca(as_variants, names, 3)
    assert sparse.coordinates.shape == (10, 1)
    assert np.array_equal(sparse.coordinates, dense.coordinates)
    assert np.array_equal(sparse.positions, positions[:1])
    rare = np.zeros((30, 5, 2), dtype=np.int8)
    with pytest.raises(ValueError, match="No variants with MAF >= 5% found for PCA"):
        fm.chromosome_pca({"genotypes": rare, "positions": np.arange(30)}, names, 2)


def test_files_match_the_oracle(fm, tmp_path):
    from ferromic import _core

    names = [f"id{i}" for i in range(30)]
    chroms = {}
    expected = {}
    for c, seed in (("1", 21), ("X", 22)):
        g = R.pybench_cohort(700, 30, seed=seed)
        positions = np.arange(700, dtype=np.int64) * 3
        chroms[c] = [(int(positions[r]), [tuple(int(v) for v in g[r, s]) for s in range(30)]) for r in range(700)]
        expected[c] = (g, positions)
    chroms["tiny"] = chroms["1"][:1]  # fewer than two variants: skipped
    out = tmp_path / "per_chr"
    fm.per_chromosome_pca(chroms, names, str(out), 4)
    assert sorted(os.listdir(out)) == ["pca_chr_1.tsv", "pca_chr_X.tsv"]
    fm.chromosome_pca_to_file(chroms["X"], names, "X", str(tmp_path), 4)
    assert (tmp_path / "pca_chr_X.tsv").read_bytes() == (out / "pca_chr_X.tsv").read_bytes()
    for c, (g, positions) in expected.items():
        res = fm.chromosome_pca(chroms[c], names, 4)
        text = (out / f"pca_chr_{c}.tsv").read_text()
        assert text == R.tsv_text(res.haplotype_labels, res.coordinates)  # byte-equal to the oracle's formatting of the GPU's coordinates
        a, w, d0, _ = cpu_pair(g, 4)
        table = np.array([[float(v) for v in line.split("\t")[1:]] for line in text.splitlines()[1:]])
        flips = np.sign((R.canonical_signs(res.coordinates) * res.coordinates).sum(axis=0))  # the column signs that canonicalise the full-precision result
        assert np.abs(table * flips - a).max() <= 32 * d0 + 0.5e-6  # six printed decimals
    combined = tmp_path / "combined.tsv"
    _core._combine_pca_results(str(out), str(combined))
    lines = combined.read_text().splitlines()
    assert lines[0] == "Haplotype\tChromosome\tPC1\tPC2\tPC3\tPC4" and len(lines) == 1 + 2 * 60
    assert lines[1].split("\t")[:2] == ["id0_L", "1"] and lines[61].split("\t")[:2] == ["id0_L", "X"]
    with pytest.raises(ValueError, match="Failed to compute PCA for any chromosome"):
        fm.per_chromosome_pca({"tiny": chroms["tiny"]}, names, str(tmp_path / "none"), 4)


def test_scale_five_populations(dev, fm):
    """1 000 samples, five populations, 4 components.  16 000 sites instead of 150 000: the thin SVD of the CPU pair costs
    4 m n^2 flops (a minute at 150 000 sites), and the haplotype count - the Gram's size - is what this case is about."""
    variants, samples = 16000, 1000
    n = 2 * samples
    g = R.pybench_cohort(variants, samples, seed=7, scale=0.08, populations=5)
    a, w, d0, kept = cpu_pair(g, 4)
    flat = g.reshape(variants, n).astype(np.uint8)
    xk = flat[kept]
    hi, lo = R.set_clear_values(xk.sum(axis=1), n)
    z = np.where(xk.T == 1, hi[None, :], lo[None, :])
    m = kept.size
    dm = dev.DeviceMatrix.from_host(flat, None, variants, samples, 2, 1)
    try:
        got = dev.pca_gram(dm, kept, hi, lo)
    finally:
        dm.close()
    assert np.array_equal(got, got.T)
    scale = 2.0 * (m + 2) * EPS / float(n - 1)
    corner = z[:256] @ z[:256].T / float(n - 1)
    assert np.all(np.abs(got[:256, :256] - corner) <= scale * (np.abs(z[:256]) @ np.abs(z[:256]).T))
    rng = np.random.default_rng(8)
    ii, jj = rng.integers(n, size=10000), rng.integers(n, size=10000)
    worst = 0.0
    for lo_i in range(0, 10000, 500):
        zi, zj = z[ii[lo_i:lo_i + 500]], z[jj[lo_i:lo_i + 500]]
        exact = (zi * zj).sum(axis=1) / float(n - 1)
        bound = scale * (np.abs(zi) * np.abs(zj)).sum(axis=1)
        err = np.abs(got[ii[lo_i:lo_i + 500], jj[lo_i:lo_i + 500]] - exact)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    print(f"scale gram: max err/bound on 10 000 entries {worst:.3e}")
    res = fm.chromosome_pca({"genotypes": g, "positions": np.arange(variants, dtype=np.int64)}, [f"s{i}" for i in range(samples)], 4)
    check_scores(res.coordinates, a, w, d0, n, "scale 16000x1000")
