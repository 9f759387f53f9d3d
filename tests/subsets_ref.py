"""Cluster decomposition restated in plain Python with itertools: the twin of the two decomposition kernels of csrc/sweep_rows.hip and csrc/sweep_support.hip and of
matcha_amd/sweep.py's subset_unrank.  No GPU, no torch; tests/test_cpu_subsets.py and tests/test_hip_subsets.py both check against it.

The rule.  A cluster table is [A, S], 2 <= S <= 32; row a holds s_a non-zero ids followed by zeros: the run before the first zero is
the cluster.  A choice is an m-subset of the POSITIONS [0, S), 1 <= m <= 8, ranked lexicographically from 0 (C(S, m) of them); the
global rank is a C(S, m) + r.  keep (complement = 0, m >= 2): the row is the ids at the chosen positions, in position order.  drop
(complement = 1): the row is the cluster's ids at all positions but the chosen ones, in position order.  A candidate is valid iff
every chosen position is < s_a, the row has at least 2 ids, the cluster's own ids are non-descending and every adjacent difference of
the row is >= min_gap.  A candidate with a chosen position >= s_a is an all-zero row, invalid; every other invalid candidate keeps
its row."""
import itertools
import math

import numpy as np

Q = 4294967296.0                                            # the support planes' fixed point: 32 fractional bits


def leading_ids(row):
    return list(itertools.takewhile(lambda v: v != 0, (int(v) for v in row)))


def choices(S, m):
    """The m-subsets of the positions [0, S) in rank order."""
    return list(itertools.combinations(range(S), m))


def count(A, S, m):
    return A * math.comb(S, m)


def candidate(cluster, S, choice, complement, min_gap):
    """(row, valid, chosen ids) of one choice of positions."""
    ids = leading_ids(cluster)
    s = len(ids)
    if any(p >= s for p in choice):
        return (), False, ()
    picked = set(choice)
    row = [ids[p] for p in range(s) if (p in picked) != bool(complement)]
    ascending = all(a <= b for a, b in zip(ids, ids[1:]))
    gaps_ok = all(not (b < a) and b - a >= min_gap for a, b in zip(row, row[1:]))
    return tuple(row), len(row) >= 2 and ascending and gaps_ok, tuple(ids[p] for p in choice)


def candidates(cluster, S, m, complement, min_gap):
    """[(row, valid)] of one cluster row of a table of width S, in rank order."""
    return [candidate(cluster, S, ch, complement, min_gap)[:2] for ch in choices(S, m)]


def table(clusters, S, m, complement, min_gap, width):
    """(rows int64 [A * C(S, m), width], invalid bool [A * C(S, m)]) of a cluster table in global-rank order."""
    rows, bad = [], []
    for cluster in clusters:
        for row, ok in candidates(cluster, S, m, complement, min_gap):
            rows.append(list(row) + [0] * (width - len(row)))
            bad.append(not ok)
    return np.asarray(rows, dtype=np.int64).reshape(-1, width), np.asarray(bad, dtype=bool)


def padded(clusters, S=None):
    """int64 [A, S]: id lists of any lengths as a zero-padded table."""
    S = max([len(c) for c in clusters] + [2]) if S is None else S
    t = np.zeros((len(clusters), S), dtype=np.int64)
    for a, c in enumerate(clusters):
        t[a, :len(c)] = c
    return t


def quantum(v):
    """rint(double(v) 2^32) of a float32 value, as the kernel takes it (round half to even)."""
    return int(np.rint(np.float64(np.float32(v)) * Q))


def support(A, S, m, values, skip, g0, vmax=1.0, state=None):
    """The support planes in integers: (sum int64 [A, S], count int64 [A, S], [n_rows, n_rejected]) after one update of rows
    g0 .. g0 + len(values) - 1 on top of ``state`` (the same triple, or None).  A row is skipped (skip != 0), rejected (NaN, negative
    or > vmax) or adds quantum(v) and 1 to the cells of its m chosen positions."""
    if state is None:
        state = (np.zeros((A, S), dtype=np.int64), np.zeros((A, S), dtype=np.int64), [0, 0])
    total, cnt, counters = state
    ch = choices(S, m)
    for i, v in enumerate(np.asarray(values, dtype=np.float32)):
        if skip is not None and skip[i]:
            continue
        if not (v >= 0 and v <= np.float32(vmax)):
            counters[1] += 1
            continue
        counters[0] += 1
        a, r = divmod(g0 + i, len(ch))
        for p in ch[r]:
            total[a, p] += quantum(v)
            cnt[a, p] += 1
    return total, cnt, counters


# ---- the g16 fixture (tests/golden/make_golden_subsets.py) ------------------------------------------------------------------------------
G16_CASES = [("keep", 3, 1, 3, (4, 9, 12, 17)), ("keep", 2, 1, 2, (3, 8, 20, 32)), ("keep", 4, 2, 8, (8, 11, 14)),
             ("drop", 1, 1, 32, (3, 9, 10, 25, 32)), ("drop", 2, 1, 20, (4, 10, 12, 20))]     # (mode, m, min_gap, width W, cluster sizes)
G16_SEED = 1600
G16_TOL = 1e-4                                              # the project's tolerance against the reference's logits


def g16_clusters(case, n_nodes=64, seed_base=G16_SEED):
    """The clusters of one case: sorted(default_rng(seed_base + case).choice(arange(1, n_nodes + 1), size, replace=False)) per size."""
    rng = np.random.default_rng(seed_base + case)
    return [sorted(int(v) for v in rng.choice(np.arange(1, n_nodes + 1), size=size, replace=False)) for size in G16_CASES[case][4]]


def g16_rows(case, clusters=None):
    """(rows int64 [sum_a C(s_a, m), W], invalid bool, offsets [A + 1]) of one case: cluster after cluster, each at its own size (the
    sweep groups clusters by size, so S = s_a), in rank order."""
    mode, m, gap, W, _ = G16_CASES[case]
    clusters = g16_clusters(case) if clusters is None else clusters
    rows, bad, off = [], [], [0]
    for cl in clusters:
        r, b = table([cl], len(cl), m, mode == "drop", gap, W)
        rows.append(r)
        bad.append(b)
        off.append(off[-1] + len(r))
    return np.concatenate(rows), np.concatenate(bad), np.asarray(off, dtype=np.int64)
