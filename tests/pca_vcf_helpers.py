"""Shared by the run_vcf --pca tests: what the PCA of a chromosome takes as input, restated from the oracle's parse
(oracle/run_vcf_ref.py: process_vcf, FLAG_PASS), and VCF cohorts with population structure written from tests/pca_ref.py's recipe.

The PCA matrix of a chromosome: every PASS variant of the chromosome's ingest, diploid - column 2 s + k is allele k of sample s,
called iff k < the length of that sample's genotype; alleles beyond the second are ignored (src/pca.rs:81-91)."""

import os
import random

import numpy as np

from oracle import run_vcf_ref as V

INT64_MAX = (1 << 63) - 1


def diploid_entries(variants, n_samples):
    """(V, S, 2) int16 of the allele of every called entry, -1 for an entry that is not called."""
    out = np.full((len(variants), n_samples, 2), -1, dtype=np.int16)
    for i, v in enumerate(variants):
        stride, data = v.genotypes.stride, v.genotypes.data
        for s in range(n_samples):
            for k in range(min(2, stride)):
                b = data[s * stride + k]
                if b == 0xFF:
                    break
                out[i, s, k] = b
    return out


def pca_input_digest(variants, n_samples):
    """FNV-1a over (8 little-endian position bytes, 2 S entry bytes with 0xFF = not called) of every variant in order."""
    g = diploid_entries(variants, n_samples)
    h = 1469598103934665603
    for i, v in enumerate(variants):
        row = np.where(g[i] < 0, 0xFF, g[i]).astype(np.uint8).reshape(-1)
        for b in list(int(v.position).to_bytes(8, "little", signed=True)) + row.tolist():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def oracle_pass_variants(kw, min_gq=30, mask_file=None, allow_file=None, exclude=(), chrom=None, region=None):
    """{chromosome: (PASS variants in order, sample names)} of a run_vcf invocation, from the oracle's parse: per chromosome the
    ingest over the union of its regions +- 3 Mb (process.rs:2011-2031), then flag == FLAG_PASS."""
    mask = V.parse_regions_file(mask_file) if mask_file else None
    allow = V.parse_regions_file(allow_file) if allow_file else None
    by_chr = {}
    if chrom is not None:
        by_chr[chrom] = [V.parse_region(region) if region else V.from_1based_inclusive(1, INT64_MAX)]
    else:
        for e in V.parse_config_file(kw["config_file"]):
            by_chr.setdefault(e.seqname, []).append(e.interval)
    out = {}
    for c in sorted(by_chr):
        try:
            seq = V.read_reference_sequence(kw["reference"], c)
            vcf_path = V.find_vcf_file(kw["vcf_folder"], c)
        except Exception:
            continue
        final_mask = {k: list(v) for k, v in (mask or {}).items()}
        final_mask.setdefault(c, []).extend(V.find_n_regions(seq))
        hulls = [(max(s - 3_000_000, 0), min(e + 3_000_000, len(seq))) for s, e in by_chr[c]]
        variants, flags, names = V.process_vcf(vcf_path, c, V.merge_intervals(hulls), min_gq, final_mask, allow, set(exclude))
        out[c] = ([v for v, f in zip(variants, flags) if f == V.FLAG_PASS], names)
    return out


def make_mixed_cohort(tmp, seed, n_samples=13):
    """Three chromosomes of every cell kind the ingest knows: missing calls (`.`, `./.`, `0|.`), haploid and triploid cells,
    multi-allelic sites, indels (discarded), low and absent GQ; a mask, an allow list.  Most sites are fully called so that PASS
    variants exist, and some of those carry a haploid or triploid cell."""
    rng = random.Random(seed)
    names = [f"POP_{'ABC'[i % 3]}_HG{i:05d}" for i in range(n_samples)]
    chroms = {"1": 5000, "7": 3500, "X": 2500}
    fasta, fai, off = "", "", 0
    for c, ln in chroms.items():
        seq = "".join(rng.choice("ACGT") for _ in range(ln))
        if c == "7":
            seq = seq[:1500] + "N" * 120 + seq[1620:]
        hdr = f">chr{c}\n"
        body = "\n".join(seq[i:i + 60] for i in range(0, ln, 60)) + "\n"
        fai += f"chr{c}\t{ln}\t{off + len(hdr)}\t60\t61\n"
        fasta += hdr + body
        off += len(hdr) + len(body)
    (tmp / "ref.fa").write_text(fasta)
    (tmp / "ref.fa.fai").write_text(fai)
    (tmp / "ann.gtf").write_text('chr1\t.\tCDS\t1\t100\t.\t+\t0\tgene_id "g"; transcript_id "t";\n')
    os.makedirs(tmp / "vcfs", exist_ok=True)
    header = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    for c, ln in chroms.items():
        lines, pos = [], 0
        while True:
            pos += rng.randint(1, 7)
            if pos > ln:
                break
            kind = rng.random()
            ref, alt = rng.choice("ACGT"), rng.choice("ACGT")
            if kind < 0.04:
                ref = "AT"
            elif kind < 0.15:
                alt = alt + "," + rng.choice("ACGT")
            site = rng.random()  # what may go wrong at this site
            f = rng.betavariate(0.8, 0.8)
            cells = []
            for i in range(n_samples):
                amax = 2 if "," in alt else 1
                a = [(rng.randint(1, amax) if rng.random() < f else 0) for _ in range(3)]
                gq = rng.choice([99, 60, 45, 31, 30])
                sep = "|" if rng.random() > 0.1 else "/"
                r = rng.random()
                if site < 0.10 and r < 0.2:
                    cells.append(rng.choice(["./.:.", ".:.", f"{a[0]}|.:{gq}", f".|{a[1]}:{gq}"]))
                elif site < 0.18 and r < 0.2:
                    cells.append(f"{a[0]}{sep}{a[1]}:{rng.choice([5, 29, '.'])}")
                elif 0.18 <= site < 0.30 and r < 0.15:
                    cells.append(f"{a[0]}:{gq}")                      # haploid: stays PASS, the site is incomplete
                elif 0.30 <= site < 0.38 and r < 0.15:
                    cells.append(f"{a[0]}|{a[1]}|{a[2]}:{gq}")        # triploid: the third allele is ignored
                elif c == "X" and i % 4 == 0 and site > 0.9:
                    cells.append(f"{a[0]}:{gq}")
                else:
                    cells.append(f"{a[0]}{sep}{a[1]}:{gq}")
            prefix = "chr" if c != "7" else ""
            lines.append(f"{prefix}{c}\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT:GQ\t" + "\t".join(cells) + "\n")
        name = {"1": "chr1.vcf", "7": "cohort.chr7.phased.vcf", "X": "chrX.vcf"}[c]
        (tmp / "vcfs" / name).write_text(header + "".join(lines))
    cfg = "seqnames\tstart\tend\tPOS\torig_ID\tverdict\tcateg\t" + "\t".join(names) + "\n"

    def row(c, s, e):
        cells = [rng.choice(["0|0", "0|1", "1|0", "1|1", "0|1_lowconf"]) for _ in range(n_samples)]
        return f"chr{c}\t{s}\t{e}\t{s}\tid\tpass\tinv\t" + "\t".join(cells) + "\n"

    cfg += row("1", 100, 2500) + row("1", 2000, 4900) + row("7", 10, 3400) + row("X", 1, 2500)
    (tmp / "config.tsv").write_text(cfg)
    (tmp / "mask.bed").write_text("chr1\t300\t420\n1\t4000\t4100\nchrX\t0\t50\n")
    (tmp / "allow.tsv").write_text("chr1\t1\t4800\nchr7\t1\t3500\nchrX\t100\t2400\n")
    return dict(vcf_folder=str(tmp / "vcfs"), reference=str(tmp / "ref.fa"), gtf=str(tmp / "ann.gtf"), config_file=str(tmp / "config.tsv")), names


def structured_genotypes(variants, samples, seed, populations=3, missing=0.01, multi=0.05, haploid=0.02, low_gq=0.003):
    """tests/pca_ref.py's benchmark recipe with population structure (scale 0.15) plus what a VCF adds: `missing` of the GENOTYPES
    are `./.` (such a site never reaches the PCA), `multi` of the rows carry one allele 2, `haploid` of the rows one haploid cell,
    `low_gq` of the rows one cell with a low GQ.  Returns (g int8 (V, S, 2), miss (V, S) bool, hap (V, S) bool, low (V, S) bool)."""
    from tests import pca_ref as R

    g = R.pybench_cohort(variants, samples, seed, scale=0.15, populations=populations).astype(np.int8)
    rng = np.random.default_rng(seed + 1)
    miss = rng.random((variants, samples)) < missing
    for r in np.nonzero(rng.random(variants) < multi)[0]:
        g[r, rng.integers(samples), rng.integers(2)] = 2
    hap = np.zeros((variants, samples), dtype=bool)
    for r in np.nonzero(rng.random(variants) < haploid)[0]:
        hap[r, rng.integers(samples)] = True
    low = np.zeros((variants, samples), dtype=bool)
    for r in np.nonzero(rng.random(variants) < low_gq)[0]:
        low[r, rng.integers(samples)] = True
    return g, miss, hap, low


def write_structured_case(tmp, chromosomes, names, seed=0):
    """chromosomes: {chr: (g, miss, hap, low)} as structured_genotypes returns them (any of the last three may be None).  Writes
    reference, GTF, one VCF per chromosome (sites 5 bp apart) and a config of two overlapping regions per chromosome."""
    rng = random.Random(seed)
    n_samples = len(names)
    fasta, fai, off = "", "", 0
    os.makedirs(tmp / "vcfs", exist_ok=True)
    header = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    cfg = "seqnames\tstart\tend\tPOS\torig_ID\tverdict\tcateg\t" + "\t".join(names) + "\n"
    for c, (g, miss, hap, low) in chromosomes.items():
        n_sites = g.shape[0]
        ln = n_sites * 5 + 100
        seq = "".join(rng.choice("ACGT") for _ in range(ln))
        hdr = f">chr{c}\n"
        body = "\n".join(seq[i:i + 60] for i in range(0, ln, 60)) + "\n"
        fai += f"chr{c}\t{ln}\t{off + len(hdr)}\t60\t61\n"
        fasta += hdr + body
        off += len(hdr) + len(body)
        txt = np.char.add(np.char.add(g[:, :, 0].astype(str), "|"), g[:, :, 1].astype(str))
        if hap is not None:
            txt = np.where(hap, g[:, :, 0].astype(str), txt)
        txt = np.where(low, np.char.add(txt, ":12"), np.char.add(txt, ":60")) if low is not None else np.char.add(txt, ":60")
        if miss is not None:
            txt = np.where(miss, "./.:.", txt)
        multi = (g > 1).any(axis=(1, 2))
        lines = [f"chr{c}\t{5 * s + 3}\t.\tA\t{'C,T' if multi[s] else 'C'}\t.\tPASS\t.\tGT:GQ\t" + "\t".join(txt[s]) + "\n" for s in range(n_sites)]
        (tmp / "vcfs" / f"chr{c}.vcf").write_text(header + "".join(lines))
        for (s, e) in ((1, ln - 1), (ln // 4, ln // 2)):
            cells = [rng.choice(["0|0", "0|1", "1|0", "1|1"]) for _ in range(n_samples)]
            cfg += f"chr{c}\t{s}\t{e}\t{s}\tid\tpass\tinv\t" + "\t".join(cells) + "\n"
    (tmp / "ref.fa").write_text(fasta)
    (tmp / "ref.fa.fai").write_text(fai)
    (tmp / "ann.gtf").write_text('chr1\t.\tCDS\t1\t100\t.\t+\t0\tgene_id "g"; transcript_id "t";\n')
    (tmp / "config.tsv").write_text(cfg)
    return dict(vcf_folder=str(tmp / "vcfs"), reference=str(tmp / "ref.fa"), gtf=str(tmp / "ann.gtf"), config_file=str(tmp / "config.tsv"))
