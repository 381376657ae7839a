"""run_vcf --pca on the GPU: one pca_chr_<chr>.tsv per chromosome under <cwd>/pca_per_chr_outputs, against tests/pca_ref.py on the
PASS variants of the oracle's parse (oracle/run_vcf_ref.py) with the Variant route's filter (variant_rule=True).

The rule and constants of tests/test_gpu_pca.py::test_files_match_the_oracle: the CPU answer is computed twice (Gram + eigh, thin
SVD), d0 is their disagreement; after fixing each column's sign against the oracle's column every printed value must be within
32 d0 + 0.5e-6 (six printed decimals).  Before the file is looked at the CPU pair must be conclusive: 32 d0 <= 1e-8 max |coordinate|
and every requested component's relative gap >= 1e-5."""

import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import pca_ref as R
from tests.pca_vcf_helpers import diploid_entries, oracle_pass_variants, structured_genotypes, write_structured_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("FERROMIC_RUN_VCF_BIN") or os.path.join(ROOT, "ferromic_amd", "bin", "run_vcf")
OUTPUTS = ("out.csv", "per_site_diversity_output.falsta.gz", "per_site_fst_output.falsta.gz", "hudson_fst_results.tsv.gz", "wc_fst_results.tsv.gz")


def run(kw, cwd, extra=(), env=None, config=True):
    """run_vcf --fst in `cwd` (created); returns (stderr, {output name: bytes of its uncompressed content})."""
    os.makedirs(cwd, exist_ok=True)
    cmd = [BIN, "--vcf_folder", kw["vcf_folder"], "--reference", kw["reference"], "--gtf", kw["gtf"], "--output_file", os.path.join(str(cwd), "out", "out.csv"), "--fst"]
    if config:
        cmd += ["--config_file", kw["config_file"]]
    res = subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=str(cwd), timeout=600, env=dict(os.environ, FERROMIC_PROGRESS="1", **(env or {})))
    assert res.returncode == 0, res.stderr[-3000:]
    files = {}
    for name in OUTPUTS:
        p = os.path.join(str(cwd), "out", name)
        if os.path.exists(p):
            files[name] = gzip.open(p, "rb").read() if name.endswith(".gz") else open(p, "rb").read()
    return res.stderr, files


def expected_scores(variants, n_samples, n_components):
    """(scores, d0, complete, kept count) of the oracle-parsed PASS variants - after the check that the CPU pair is conclusive."""
    g = diploid_entries(variants, n_samples)
    kept, complete = R.site_filter(g, variant_rule=True)
    x = R.haplotype_matrix(g, kept)
    k = min(R.clamp_components(n_components, complete, x.shape[0]), kept.size)
    a, w = R.transform(x, k)
    b = R.transform_svd(x, k)
    b = b * np.sign((a * b).sum(axis=0))
    d0 = float(np.abs(a - b).max())
    assert 32 * d0 <= 1e-8 * np.abs(a).max(), ("CPU pair inconclusive", d0)
    gaps = (w[:k] - w[1:k + 1]) / w[0]
    assert gaps.min() >= 1e-5, ("spectral gap too small for this cohort", gaps)
    return a, d0, complete, int(kept.size), len(variants)


def check_file(path, names, variants, n_components, what):
    n_samples = len(names)
    a, d0, complete, kept, total = expected_scores(variants, n_samples, n_components)
    lines = open(path).read().splitlines()
    k = min(n_components, complete, 2 * n_samples)
    assert lines[0] == "Haplotype" + "".join(f"\tPC{i + 1}" for i in range(k)), lines[0]
    assert [ln.split("\t")[0] for ln in lines[1:]] == [f"{s}_{side}" for s in names for side in "LR"]
    table = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]])
    assert table.shape == a.shape == (2 * n_samples, k)
    flips = np.sign((table * a).sum(axis=0))
    err = float(np.abs(table * flips - a).max())
    print(f"{what}: {total} PASS variants, {complete} complete, {kept} kept, {k} components: err {err:.3e}, allowance {32 * d0 + 0.5e-6:.3e} (32 d0 = {32 * d0:.3e})")
    assert err <= 32 * d0 + 0.5e-6, (what, err, d0)
    return complete, kept, total


def two_chromosome_case(tmp_path, samples=40, exclude=False):
    names = [f"POP{i % 3}_S{i:03d}" for i in range(samples)]
    chroms = {"1": structured_genotypes(3000, samples, 61, populations=3), "X": structured_genotypes(2400, samples, 62, populations=4)}
    return write_structured_case(tmp_path, chroms, names, seed=5), names


@pytest.fixture(scope="module")
def shared_case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pca_case")
    kw, names = two_chromosome_case(tmp)
    return tmp, kw, names, oracle_pass_variants(kw)


def test_files_match_the_oracle_and_other_outputs_do_not_change(shared_case):
    tmp, kw, names, oracle = shared_case
    stderr, with_pca = run(kw, tmp / "with", ["--pca", "--pca_components", "4", "--pca_output", "unused.tsv"])
    _, without = run(kw, tmp / "without")
    out = tmp / "with" / "pca_per_chr_outputs"
    assert sorted(os.listdir(out)) == ["pca_chr_1.tsv", "pca_chr_X.tsv"]
    assert not (tmp / "without" / "pca_per_chr_outputs").exists() and not (tmp / "with" / "out" / "pca_per_chr_outputs").exists()
    assert not (tmp / "with" / "unused.tsv").exists()
    for c in ("1", "X"):
        variants, sample_names = oracle[c]
        assert sample_names == names
        complete, kept, total = check_file(out / f"pca_chr_{c}.tsv", names, variants, 4, f"chr{c}")
        assert complete < total  # haploid cells among the PASS variants
        assert f"Found {complete} variants with complete data out of {total} total variants" in stderr
        assert f"Keeping {kept}/{complete} variants with MAF >= 5% for PCA" in stderr
    assert "is ignored" not in stderr and "PCA error" not in stderr
    # CSV, FALSTA and TSV outputs: byte for byte the run without --pca
    # (wc_fst_results.tsv.gz appears only with --fst_populations: whatever one run writes the other must write too)
    assert set(with_pca) == set(without) and set(OUTPUTS[:4]) <= set(with_pca), (sorted(with_pca), sorted(without))
    for name in without:
        assert with_pca[name] == without[name], name


def test_default_components_and_exclusion(shared_case):
    tmp, kw, names, _ = shared_case
    stderr, _ = run(kw, tmp / "default", ["--pca", "--exclude", names[7]], env={"FERROMIC_TIMING": "1"})
    oracle = oracle_pass_variants(kw, exclude=[names[7]])
    kept_names = [s for s in names if s != names[7]]
    for c in ("1", "X"):
        variants, sample_names = oracle[c]
        assert sample_names == kept_names
        path = tmp / "default" / "pca_per_chr_outputs" / f"pca_chr_{c}.tsv"
        assert open(path).readline().count("\tPC") == 10
        check_file(path, kept_names, variants, 10, f"chr{c}, 10 components, one sample excluded")
    assert "[TIMING] pca " in stderr


def test_single_chromosome_mode(shared_case):
    tmp, kw, names, _ = shared_case
    run(kw, tmp / "chr_mode", ["--chr", "X", "--region", "2000-9000", "--pca", "--pca_components", "3"], config=False)
    assert os.listdir(tmp / "chr_mode" / "pca_per_chr_outputs") == ["pca_chr_X.tsv"]
    variants, sample_names = oracle_pass_variants(kw, chrom="X", region="2000-9000")["X"]
    assert sample_names == names and len(variants) > 1000  # the ingest hull is the region +- 3 Mb: the whole chromosome
    check_file(tmp / "chr_mode" / "pca_per_chr_outputs" / "pca_chr_X.tsv", names, variants, 3, "--chr X --region")


def test_chromosomes_without_a_pca_do_not_fail_the_run(tmp_path):
    samples = 24
    names = [f"S{i:03d}" for i in range(samples)]
    good = structured_genotypes(1500, samples, 71, populations=3)
    rare = np.zeros((400, samples, 2), dtype=np.int8)
    rare[np.arange(400), np.arange(400) % samples, 0] = 1                # singletons: MAF 1 / 48 < 5 %
    g2, _, _, _ = structured_genotypes(300, samples, 72)
    no_pass = (g2, None, None, np.ones((300, samples), dtype=bool))       # every cell has a low GQ
    g3, _, _, _ = structured_genotypes(300, samples, 73, multi=0.0)
    all_haploid = (g3, None, np.ones((300, samples), dtype=bool), None)
    kw = write_structured_case(tmp_path, {"1": good, "2": (rare, None, None, None), "3": no_pass, "4": all_haploid}, names, seed=9)
    stderr, files = run(kw, tmp_path / "run", ["--pca", "--pca_components", "4"])
    assert os.listdir(tmp_path / "run" / "pca_per_chr_outputs") == ["pca_chr_1.tsv"]
    assert "[WARN] Chromosome 2 PCA error: Parse error: No variants with MAF >= 5% found for PCA" in stderr
    assert "[WARN] No filtered variants remain for chromosome 3. Skipping PCA." in stderr
    assert "[WARN] Chromosome 4 PCA error: Parse error: No variants with MAF >= 5% found for PCA" in stderr
    assert "Found 0 variants with complete data out of 300 total variants" in stderr
    variants, sample_names = oracle_pass_variants(kw)["1"]
    check_file(tmp_path / "run" / "pca_per_chr_outputs" / "pca_chr_1.tsv", names, variants, 4, "the chromosome that has a PCA")
    assert files["out.csv"].count(b"\n") >= 1 + 2  # the regions of the other chromosomes are still reported


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_sharded_over_devices(shared_case, devices):
    """--devices lists one GPU several times: the in-process transport, every PASS matrix split into site slabs."""
    tmp, kw, names, oracle = shared_case
    where = tmp / ("dev" + devices.replace(",", ""))
    stderr, _ = run(kw, where, ["--pca", "--pca_components", "4", "--devices", devices], env={"FERROMIC_SHARD_MIN_BYTES": "1"})
    assert "PCA error" not in stderr, stderr[-2000:]
    for c in ("1", "X"):
        check_file(where / "pca_per_chr_outputs" / f"pca_chr_{c}.tsv", names, oracle[c][0], 4, f"chr{c} --devices {devices}")


def test_sharded_when_the_first_slab_keeps_no_site(tmp_path):
    samples = 30
    names = [f"S{i:03d}" for i in range(samples)]
    g, miss, hap, low = structured_genotypes(3000, samples, 81, populations=3)
    g[:1100] = 0  # the first third of the positions is monomorphic: slab 0 of three contributes zeros to the Gram
    kw = write_structured_case(tmp_path, {"1": (g, miss, hap, low)}, names, seed=3)
    stderr, _ = run(kw, tmp_path / "run", ["--pca", "--pca_components", "4", "--devices", "0,0,0"], env={"FERROMIC_SHARD_MIN_BYTES": "1"})
    assert "PCA error" not in stderr, stderr[-2000:]
    variants, _ = oracle_pass_variants(kw)["1"]
    third = len(variants) // 3
    kept, _ = R.site_filter(diploid_entries(variants, samples), variant_rule=True)
    assert kept.size > 100 and kept.min() >= ((len(variants) + 63) // 64 // 3) * 64, (kept.min(), third)  # no kept site in slab 0
    check_file(tmp_path / "run" / "pca_per_chr_outputs" / "pca_chr_1.tsv", names, variants, 4, "first slab without kept sites")


def test_chromosome_above_the_row_table_threshold(tmp_path):
    """4 500 variants, of which more than 4 096 are PASS: the chromosome's matrix is uploaded with its per-row tables (row_gap / row_hi,
    built from 4 096 rows up), so the site scan skips the called plane of complete rows and the upper plane of biallelic ones - what every
    real chromosome does.  `./.` cells are rare here (a site with one is not PASS); the uncalled entries of the PCA matrix are the second
    alleles of haploid cells.  FMH_ROW_HI=0 (no tables) must write the same bytes."""
    samples = 40
    names = [f"POP{i % 3}_S{i:03d}" for i in range(samples)]
    g, miss, hap, low = structured_genotypes(4500, samples, 91, populations=3, missing=0.0005)
    kw = write_structured_case(tmp_path, {"1": (g, miss, hap, low)}, names, seed=11)
    variants, sample_names = oracle_pass_variants(kw)["1"]
    assert sample_names == names
    # not vacuous, on the oracle's parse alone: enough PASS rows for the tables, rows the filter must refuse, mostly clean rows
    entries = diploid_entries(variants, samples).reshape(len(variants), -1)
    uncalled, high = (entries < 0).any(axis=1), (entries > 1).any(axis=1)
    assert 4096 <= len(variants) < 4500 and miss.any()
    assert uncalled.sum() >= 50 and high.sum() >= 150 and (uncalled & high).sum() >= 1 and (~(uncalled | high)).sum() * 2 > len(variants)
    freq = np.clip(entries[uncalled | high], 0, 1).sum(axis=1) / (2.0 * samples)
    assert (np.minimum(freq, 1.0 - freq) >= 0.1).sum() >= 50  # refused for their flag alone: a flag the scan missed would keep them
    args = ["--pca", "--pca_components", "4"]
    stderr, _ = run(kw, tmp_path / "tables", args)
    path = tmp_path / "tables" / "pca_per_chr_outputs" / "pca_chr_1.tsv"
    complete, kept, total = check_file(path, names, variants, 4, "chr1, 4 500 variants")
    assert total == len(variants) and complete < total
    assert f"Found {complete} variants with complete data out of {total} total variants" in stderr
    assert f"Keeping {kept}/{complete} variants with MAF >= 5% for PCA" in stderr
    assert "PCA error" not in stderr
    stderr0, _ = run(kw, tmp_path / "no_tables", args, env={"FMH_ROW_HI": "0"})
    assert f"Keeping {kept}/{complete} variants with MAF >= 5% for PCA" in stderr0
    assert (tmp_path / "no_tables" / "pca_per_chr_outputs" / "pca_chr_1.tsv").read_bytes() == path.read_bytes()
