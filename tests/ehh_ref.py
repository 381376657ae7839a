"""Numpy oracle of the extended haplotype homozygosity scans, written from the definition in include/ferromic_hip.h and sharing nothing with
the kernel.

A cohort is an allele matrix x [rows][cols] (uint8, alleles 0..7) and a called matrix [rows][cols] (bool) or None = everything called; a
group is a boolean column mask with n members.  An entry's state is its allele, or 255 when it is not called.  Per item (focal row, side) the
rows are walked outward and the members' labels refined with np.unique over (label, state) pairs; the pair counts of the two cores come from
np.bincount; the stop rules run in Python ints.  The statistics are float(a) / float(b) and math.log.

brute_pair_steps is a second, independent definition (per pair of members, the length of the flank they share) that pins the oracle itself;
mosaic() builds the cohorts with linkage the tests need (columns drawn independently agree over a handful of rows only)."""

import math

import numpy as np

SIDE_DTYPE = np.dtype([("area2", np.uint64, (2,)), ("pair_steps", np.uint64, (2,)), ("steps", np.uint32, (2,)), ("core", np.uint32, (2,)),
                       ("flags", np.uint32), ("reserved", np.uint32)])
EDGE0, EDGE1, GAP0, GAP1, SKIPPED = 1, 2, 4, 8, 16


def states(x, called):
    return np.asarray(x, dtype=np.uint8) if called is None else np.where(called, x, 255).astype(np.uint8)


def mosaic(rows, cols, founders=6, switch=0.01, mutation=0.002, seed=0, freq=0.5):
    """[rows][cols] uint8: every column copies one of `founders` random haplotypes, switches founder with probability `switch` per row and
    flips an allele with probability `mutation`."""
    rng = np.random.default_rng(seed)
    base = (rng.random((rows, founders)) < freq).astype(np.uint8)
    jumps = rng.random((rows, cols)) < switch
    jumps[0] = True
    draws = rng.integers(0, founders, size=(rows, cols))
    last = np.maximum.accumulate(np.where(jumps, np.arange(rows)[:, None], 0), axis=0)  # the row of each entry's latest switch
    source = draws[last, np.arange(cols)[None, :]]
    x = base[np.arange(rows)[:, None], source]
    return x ^ (rng.random((rows, cols)) < mutation).astype(np.uint8)


def pairs_of(label, core_of_label):
    """(P_0, P_1): unordered pairs inside the classes, per core, as Python ints."""
    sizes = np.bincount(label)
    out = [0, 0]
    for cls, c in enumerate(sizes.tolist()):
        out[core_of_label[cls]] += c * (c - 1) // 2
    return out


def item(state, members, f, side, row_begin, row_end, x_of, num, den, max_extent, max_gap, min_core):
    """One (focal, side): (dict of the record's fields as Python ints, the two curves [P_a(1), .., P_a(steps_a)])."""
    at_focal = state[f, members]
    core = np.where(at_focal == 0, 0, np.where(at_focal == 1, 1, 2))
    n_core = [int((core == 0).sum()), int((core == 1).sum())]
    rec = dict(area2=[0, 0], pair_steps=[0, 0], steps=[0, 0], core=n_core, flags=0)
    curves = [[], []]
    if min(n_core) < min_core:
        rec["flags"] = SKIPPED
        return rec, curves
    who = np.nonzero(core < 2)[0]  # members of neither core count nowhere
    label = core[who].astype(np.int64)
    label = np.unique(label, return_inverse=True)[1].reshape(-1)
    core_of_label = sorted(set(core[who].tolist()))
    p_init = [c * (c - 1) // 2 for c in n_core]
    alive = [p > 0 for p in p_init]
    prev = list(p_init)
    d = 0
    while any(alive):
        d += 1
        row = f + side * d
        if (max_extent and d > max_extent) or row < row_begin or row >= row_end:
            break
        gap = abs(x_of(row) - x_of(row - side))
        pair = label * 256 + state[row, members[who]].astype(np.int64)
        uniq, label = np.unique(pair, return_inverse=True)
        label = label.reshape(-1)
        core_of_label = [core_of_label[int(u) // 256] for u in uniq]
        p = pairs_of(label, core_of_label)
        for a in (0, 1):
            if not alive[a]:
                continue
            if max_gap > 0 and gap > max_gap:
                rec["flags"] |= GAP0 << a
                alive[a] = False
            elif p[a] * den < p_init[a] * num:
                alive[a] = False
            else:
                rec["area2"][a] += (prev[a] + p[a]) * gap
                rec["pair_steps"][a] += p[a]
                rec["steps"][a] = d
                curves[a].append(p[a])
                if p[a] == 0:
                    alive[a] = False
        prev = p
    for a in (0, 1):
        if alive[a]:
            rec["flags"] |= EDGE0 << a
    return rec, curves


def scan(x, called, mask, focal, row_begin=0, row_end=None, positions=None, min_ehh=(0, 1), max_extent=0, max_gap=0, min_core=0, curve=False):
    """Every (focal, side): (sides [F][2] of SIDE_DTYPE with the left side first, pairs [F][2][2][max_extent] uint32 or None)."""
    state = states(x, called)
    members = np.nonzero(np.asarray(mask, dtype=bool))[0]
    row_end = state.shape[0] if row_end is None else row_end
    x_of = (lambda r: int(r)) if positions is None else (lambda r: int(positions[r]))
    focal = [int(f) for f in focal]
    sides = np.zeros((len(focal), 2), dtype=SIDE_DTYPE)
    pairs = np.zeros((len(focal), 2, 2, max_extent), dtype=np.uint32) if curve else None
    for i, f in enumerate(focal):
        for s, side in enumerate((-1, 1)):
            rec, curves = item(state, members, f, side, row_begin, row_end, x_of, int(min_ehh[0]), int(min_ehh[1]), max_extent, max_gap, min_core)
            for key in ("area2", "pair_steps", "steps", "core", "flags"):
                sides[i, s][key] = rec[key]
            if curve:
                for a in (0, 1):
                    pairs[i, s, a, : len(curves[a])] = curves[a]
    return sides, pairs


def stats(sides, include_edges=False):
    """dict of ihh [F][2], sl [F][2], ihs [F], nsl [F] (float64, NaN where the header says so)."""
    sides = np.asarray(sides).reshape(-1, 2)
    count = sides.shape[0]
    out = dict(ihh=np.full((count, 2), np.nan), sl=np.full((count, 2), np.nan), ihs=np.full(count, np.nan), nsl=np.full(count, np.nan))
    for i in range(count):
        left, right = sides[i, 0], sides[i, 1]
        flags = int(left["flags"]) | int(right["flags"])
        usable = not (flags & SKIPPED) and (include_edges or not (flags & (EDGE0 | EDGE1 | GAP0 | GAP1)))
        for a in (0, 1):
            n_a = int(left["core"][a])
            p_init = n_a * (n_a - 1) // 2
            if usable and p_init > 0:
                out["ihh"][i, a] = float(int(left["area2"][a]) + int(right["area2"][a])) / float(2 * p_init)
                out["sl"][i, a] = float(p_init + int(left["pair_steps"][a]) + int(right["pair_steps"][a])) / float(p_init)
        for key, source in (("ihs", "ihh"), ("nsl", "sl")):
            one, zero = float(out[source][i, 1]), float(out[source][i, 0])
            if one > 0.0 and zero > 0.0:
                out[key][i] = math.log(one / zero)
    return out


def brute_pair_steps(x, called, mask, f, side, row_begin, row_end, max_extent=0):
    """pair_steps of both cores without a threshold or a gap rule, from the second definition: the sum over the unordered pairs of a core of
    the number of flanking rows, counted outward from the focal row and inside the range and max_extent, over which the two members agree."""
    state = states(x, called)
    members = np.nonzero(np.asarray(mask, dtype=bool))[0]
    limit = (row_end - 1 - f) if side > 0 else (f - row_begin)
    if max_extent:
        limit = min(limit, max_extent)
    out = [0, 0]
    for a in (0, 1):
        who = [int(m) for m in members if state[f, m] == a]
        for i in range(len(who)):
            for j in range(i + 1, len(who)):
                d = 0
                while d < limit and state[f + side * (d + 1), who[i]] == state[f + side * (d + 1), who[j]]:
                    d += 1
                out[a] += d
    return out
