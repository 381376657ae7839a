"""The table form of the tiled sweep's plan (plan_prefix, ferromic_amd/csrc/sweep_plan.hpp) against its definition, on the CPU.

`sweep_plan_check prefix` prints, for groups given as column ranges on matrices that hold the prefix counts, whether the plan answers the
counted groups from the table and, per counted group, the two boundaries whose entries it subtracts and the at most two edge vectors it still
reads with their masks.  Nothing here is a recorded answer: every line is checked against what the table form must compute -

  * on random rows of bits, P[b_hi] - P[b_lo] plus the masked popcounts of the edge vectors IS the number of set bits in [c0, c1), where P[b]
    counts the row's columns before 128 b and P[last boundary] stops at the row's last column (the bits past it are set in the test rows);
  * P[0] is never loaded (b = 0 stands for "no load"), a range without a whole vector loads no entry, an edge is a vector the range covers
    partly, and there are as many edges as such vectors: widths 0, 1 and 2;
  * the table form is taken exactly when the route is the tiled one, the table exists, the option is on and every counted group is one range;
    the window and the derived group are what they are without the table.
"""

import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lines():
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), "plan_check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    run = subprocess.run([os.path.join(ROOT, "ferromic_amd", "bin", "sweep_plan_check"), "prefix"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.splitlines()


def parse(line):
    f = line.split("\t")
    what, w, c, m, groups = f[0].split("/")
    rec = {"what": what, "pvec": int(w[1:]), "columns": int(c[1:]), "mode": int(m[1:]),
           "groups": [[tuple(int(x) for x in r.split("-")) for r in g.split("+")] for g in groups.split("|")],
           "status": int(f[1]), "route": f[2], "tiled": int(f[3]), "prefix": int(f[4]), "vecs": int(f[5]), "first": int(f[6]), "count": int(f[7]),
           "derived": int(f[8]), "counted": []}
    for g in f[9:]:
        parts = g.split(",")
        edges = []
        for e in parts[3:]:
            v, mask = e.split(":")
            edges.append((int(v), [int(x, 16) for x in mask.split(".")]))
        rec["counted"].append({"b_lo": int(parts[0]), "b_hi": int(parts[1]), "n_edges": int(parts[2]), "edges": edges})
    return rec


def partial_vectors(c0, c1, columns):
    """The vectors of which [c0, c1) holds some but not all of the row's columns."""
    out = []
    for v in range(c0 // 128, (c1 - 1) // 128 + 1):
        lo, hi = 128 * v, min(128 * v + 128, columns)
        inside = min(c1, hi) - max(c0, lo)
        if 0 < inside < hi - lo:
            out.append(v)
    return out


def check_group(pg, c0, c1, pvec, columns, rng, name):
    assert 0 <= pg["b_lo"] <= pg["b_hi"] <= pvec, name
    assert pg["b_lo"] < pg["b_hi"] or pg["b_lo"] == pg["b_hi"] == 0, name  # nothing whole: no entry is loaded
    edges = pg["edges"][:pg["n_edges"]]
    assert sorted(v for v, _ in edges) == partial_vectors(c0, c1, columns), name
    for v, mask in pg["edges"][pg["n_edges"]:]:
        assert v == 0 and mask == [0, 0, 0, 0], name
    for _ in range(8):
        bits = np.zeros(pvec * 128, dtype=np.int64)
        bits[:columns] = rng.integers(0, 2, size=columns)
        truth = int(bits[c0:c1].sum())
        bits[columns:] = 1  # the table must not count them; a mask must not keep them
        prefix = [int(bits[:min(128 * b, columns)].sum()) for b in range(pvec + 1)]
        got = prefix[pg["b_hi"]] - prefix[pg["b_lo"]]
        for v, mask in edges:
            for k in range(4):
                word = bits[128 * v + 32 * k:128 * v + 32 * k + 32]
                got += sum(int(word[b]) for b in range(32) if mask[k] >> b & 1)
        assert got == truth, (name, got, truth)


def test_table_form_plans():
    recs = [parse(x) for x in lines()]
    assert len(recs) > 90
    rng = np.random.default_rng(1)
    seen_widths = set()
    for r in recs:
        name = (r["what"], r["pvec"], r["groups"])
        assert r["status"] == 0, name
        contiguous = [len(g) == 1 for g in r["groups"]]
        counted = [i for i in range(len(r["groups"])) if i != r["derived"]]
        want = (r["what"] in ("one", "two", "split", "default") and r["tiled"] == 1 and len(counted) > 0 and all(contiguous[i] for i in counted))
        assert r["prefix"] == int(want), name
        if not r["prefix"]:
            assert r["vecs"] == 0 and not r["counted"], name
            continue
        assert r["route"] == "tiled" and len(r["counted"]) == len(counted), name
        total = 0
        for pg, i in zip(r["counted"], counted):
            (c0, c1), = r["groups"][i]
            check_group(pg, c0, c1, r["pvec"], r["columns"], rng, name)
            total += pg["n_edges"]
            seen_widths.add(pg["n_edges"])
        assert r["vecs"] == total, name
    assert seen_widths == {0, 1, 2}


def test_named_cases():
    """The cases the design names, spelled out: the benchmark's split, a range of whole vectors, a range that ends on a vector boundary."""
    by = {}
    for x in lines():
        r = parse(x)
        by[r["what"], r["pvec"], tuple(tuple(g) for g in r["groups"])] = r
    r = by["two", 40, (((0, 2500),), ((2500, 5115),))]  # group 1 derived, group 0: P[19] and the 68 columns of vector 19
    assert (r["prefix"], r["vecs"], r["first"], r["count"], r["derived"]) == (1, 1, 0, 20, 1)
    assert r["counted"][0]["b_lo"] == 0 and r["counted"][0]["b_hi"] == 19 and r["counted"][0]["edges"][0] == (19, [0xFFFFFFFF, 0xFFFFFFFF, 0xF, 0])
    r = by["two", 40, (((0, 2560),), ((2560, 5115),))]  # ends on a boundary: one entry, no vector
    assert (r["prefix"], r["vecs"]) == (1, 0) and (r["counted"][0]["b_lo"], r["counted"][0]["b_hi"]) == (0, 20)
    r = by["one", 3, (((128, 256),),)]  # whole vectors only: two entries
    assert (r["prefix"], r["vecs"]) == (1, 0) and (r["counted"][0]["b_lo"], r["counted"][0]["b_hi"]) == (1, 2)
    r = by["one", 3, (((130, 140),),)]  # inside one vector: no entry
    assert (r["prefix"], r["vecs"]) == (1, 1) and (r["counted"][0]["b_lo"], r["counted"][0]["b_hi"]) == (0, 0)
    r = by["one", 40, (((0, 5115),),)]  # the whole row: nothing is counted, the row totals answer (no table form)
    assert (r["prefix"], r["derived"]) == (0, 0)
    r = by["one", 40, (((4991, 5115),),)]  # to the row's end: the last boundary is the row total, no second edge
    assert (r["prefix"], r["vecs"]) == (1, 1) and (r["counted"][0]["b_lo"], r["counted"][0]["b_hi"]) == (39, 40)
    assert by["off", 40, (((0, 2500),), ((2500, 5115),))]["prefix"] == 0
    assert by["notable", 40, (((0, 2500),), ((2500, 5115),))]["prefix"] == 0
    assert by["split", 40, (((0, 100), (200, 300)), ((1000, 2000),))]["prefix"] == 0
