"""Cluster completion restated in plain Python with itertools: the twin of csrc/sweep_rows.hip's kway_complete_rows_kernel and
of matcha_amd/sweep.py's completion_unrank.  No GPU, no torch; tests/test_cpu_complete.py and tests/test_hip_complete.py both check against it.

The rule.  A cluster row holds s non-zero ids followed by zeros: the run before the first zero is the cluster.  The free parts are the
ascending f-tuples of [lo, lo + n) whose adjacent differences are all >= min_gap, in lexicographic order: their position is the free
rank.  The candidate of (cluster, free part) is the s + f ids sorted ascending, duplicates kept, zero-padded to the width.  It is valid
iff s >= 1, the cluster's own ids are non-descending and every adjacent difference of the row is >= min_gap.  A cluster that descends
somewhere is not merged: the row is its ids in their order followed by the free part, and it is invalid."""
import functools
import itertools

import numpy as np


@functools.lru_cache(maxsize=None)
def free_parts(lo, n, f, min_gap):
    """The free parts in rank order (cached: the callers only read the list)."""
    return [c for c in itertools.combinations(range(lo, lo + n), f) if all(b - a >= min_gap for a, b in zip(c, c[1:]))]


def leading_ids(row):
    return list(itertools.takewhile(lambda v: v != 0, (int(v) for v in row)))


def candidates(cluster, lo, n, f, min_gap):
    """[(row, valid)] of one cluster row, in free-rank order."""
    ids = leading_ids(cluster)
    ascending = all(a <= b for a, b in zip(ids, ids[1:]))
    out = []
    for part in free_parts(lo, n, f, min_gap):
        row = sorted(ids + list(part)) if ascending else ids + list(part)
        gaps_ok = all(not (b < a) and b - a >= min_gap for a, b in zip(row, row[1:]))
        out.append((tuple(row), len(ids) >= 1 and ascending and gaps_ok))
    return out


def count(A, n, f, min_gap):
    return A * len(free_parts(0, n, f, min_gap))


def table(clusters, lo, n, f, min_gap, width):
    """(rows int64 [A * C_f, width], invalid bool [A * C_f]) of a cluster table in global-rank order."""
    rows, bad = [], []
    for cluster in clusters:
        for row, ok in candidates(cluster, lo, n, f, min_gap):
            rows.append(list(row) + [0] * (width - len(row)))
            bad.append(not ok)
    return np.asarray(rows, dtype=np.int64).reshape(-1, width), np.asarray(bad, dtype=bool)


def padded(clusters, S=None):
    """int64 [A, S]: id lists of any lengths as a zero-padded table."""
    S = max([len(c) for c in clusters] + [1]) if S is None else S
    t = np.zeros((len(clusters), S), dtype=np.int64)
    for a, c in enumerate(clusters):
        t[a, :len(c)] = c
    return t


# ---- the g15 fixture (tests/golden/make_golden_complete.py) -----------------------------------------------------------------------------
G15_CASES = [(1, 1, 1, 32, (1, 3, 7, 8, 9, 15, 24, 31)), (2, 2, 1, 32, (1, 2, 6, 7, 8, 13, 22, 30)), (0, 1, 1, 9, (1, 4, 8)),
             (3, 2, 2, 16, (1, 2, 6, 9, 12, 14))]          # (chromosome, free, min_gap, width, cluster sizes)
G15_SEED = 1500
G15_TOL = 1e-4                                              # the project's tolerance against the reference's logits


def g15_clusters(case, n_nodes=64, seed_base=G15_SEED):
    """The clusters of one case: default_rng(seed_base + case); each a sorted size-subset of 1 .. n_nodes - (size - 1)(min_gap - 1),
    stretched by j (min_gap - 1), so the cluster itself keeps the gap."""
    _, _, min_gap, _, sizes = G15_CASES[case]
    rng = np.random.default_rng(seed_base + case)
    out = []
    for size in sizes:
        top = n_nodes - (size - 1) * (min_gap - 1)
        ids = np.sort(rng.choice(np.arange(1, top + 1), size=size, replace=False)) + np.arange(size) * (min_gap - 1)
        out.append([int(v) for v in ids])
    return out


def k_sel(valid_logits):
    """(K_a, gap): the K in [2, min(8, valid - 1)] behind which the logits, sorted downwards, have their largest gap."""
    s = np.sort(np.asarray(valid_logits, dtype=np.float64))[::-1]
    hi = min(8, len(s) - 1)
    assert hi >= 2
    gaps = s[1:hi] - s[2:hi + 1]                               # gaps[j]: between the K = j + 2 best and the next
    j = int(np.argmax(gaps))
    return j + 2, float(gaps[j])
