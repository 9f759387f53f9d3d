"""The anchored k-way sweep without a GPU (matcha_amd/sweep.py, the host side of csrc/sweep_rows.hip and csrc/sweep_select.hip): the anchored candidate
rule and its ranking against itertools, argument errors refused before any device call, and that the g11 fixture separates every
anchor's top rows by far more than the tolerance its GPU test allows."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from matcha_amd import _lib
from matcha_amd import sweep as SW
from tests.helpers import gold
from tests.test_cpu_kway import G11_TOL, brute

REGIONS = [(1, 12), (5, 16)]
GRID = [(lo, n, k, s, g) for lo, n in REGIONS for k in (2, 3, 4, 5) for s in range(1, k) for g in (1, 2, 3)]
PAIR_OFFSETS = [(0, 5), (3, 9), (7, 15)]          # anchor pairs of the g11 comparison, as offsets into the case's chromosome
CLOSE_PAIR = (2, 3)                               # closer than the gap in both cases that have pairs (min_gap 2 and 3)


def anchor_cases(lo, n, s, g):
    """Anchor rows of s ids for the region [lo, lo + n): name -> row."""
    hi = lo + n
    above = [hi + 3 + 3 * j for j in range(s)]                           # clear of the region by more than any gap
    cases = {"inside": [lo + 2 + 3 * j for j in range(s)], "above": above,
             "edge_above": [hi] + above[:s - 1]}                         # one past the region's end: within the gap of its last node
    if lo >= 2:
        cases["edge_below"] = [lo - 1] + above[:s - 1]
    if lo >= 4:
        cases["below"] = [lo - 3] + above[:s - 1]                        # s > 1: one below and the others above
    if s >= 2:
        cases["in_and_out"] = [lo + 4] + above[:s - 1]
        cases["unsorted"] = cases["inside"][::-1]                        # an anchor row is a set: the candidate is sorted
        cases["too_close"] = [lo + 3, lo + 3 + g - 1] + above[:s - 2]    # breaks the rule itself (g = 1: a repeated id)
    return cases


def brute_anchored(anchor, lo, n, k, g):
    """The rule restated: for every free part (brute, size k - s, in its lexicographic order) the sorted union and its validity."""
    out = []
    for free in brute(lo, n, k - len(anchor), g):
        row = tuple(sorted(list(anchor) + list(free)))
        out.append((row, all(b - a >= g for a, b in zip(row, row[1:]))))
    return out


def test_count_and_unrank_match_itertools():
    seen = set()
    universe = {}
    for lo, n, k, s, g in GRID:
        f = k - s
        cf = len(brute(lo, n, f, g))
        assert cf == (n if f == 1 else SW.kway_count(n, f, g))
        for A in (0, 1, 5):
            assert SW.anchored_count(A, s, n, k, g) == A * cf
        if (lo, n, k, g) not in universe:                                # every candidate of size k over the region and all anchors
            universe[lo, n, k, g] = np.asarray(brute(1, lo + n + 3 * k - 3, k, g), dtype=np.int64)      # up to the largest anchor id
        for name, anchor in anchor_cases(lo, n, s, g).items():
            ref = brute_anchored(anchor, lo, n, k, g)
            got = [SW.anchored_unrank(r, anchor, lo, n, k, g) for r in range(cf)]
            assert got == ref, (lo, n, k, s, g, name)                    # every rank round-trips
            for bad in (-1, cf):
                with pytest.raises(IndexError):
                    SW.anchored_unrank(bad, anchor, lo, n, k, g)
            valid = [row for row, ok in got if ok]
            if name == "too_close":
                assert not valid
            # the valid rows, in rank order, are exactly the candidates that contain the anchor and take the rest from the region
            U = universe[lo, n, k, g]
            fixed = np.isin(U, anchor)
            keep = (fixed.sum(axis=1) == s) & (fixed | ((U >= lo) & (U < lo + n))).all(axis=1)
            assert valid == [tuple(c) for c in U[keep].tolist()], (lo, n, k, s, g, name)
            if valid:
                seen.add(name)
            if f == 1:
                seen.add("f1")
                assert [row for row, _ in got] == [tuple(sorted(anchor + [v])) for v in range(lo, lo + n)]
    assert seen == {"inside", "above", "edge_above", "edge_below", "below", "in_and_out", "unsorted", "f1"}
    # a free node on an anchor or within the gap of it is invalid and keeps its rank
    assert SW.anchored_unrank(3, [4], 1, 12, 2, 1) == ((4, 4), False)
    assert SW.anchored_unrank(4, [4], 1, 12, 2, 2) == ((4, 5), False) and SW.anchored_unrank(5, [4], 1, 12, 2, 2) == ((4, 6), True)
    assert SW.anchored_unrank(11, [13], 1, 12, 2, 2) == ((12, 13), False) and SW.anchored_unrank(11, [13], 1, 12, 2, 1) == ((12, 13), True)


def test_library_count_host_only():
    lib = _lib.load()
    for lo, n, k, s, g in GRID:
        for A in (0, 1, 7):
            assert lib.matcha_kway_anchor_count(A, s, n, k, g) == SW.anchored_count(A, s, n, k, g)
    cf = math.comb(2491, 4)
    assert cf > 1 << 40
    A = ((1 << 63) - 1) // cf
    assert lib.matcha_kway_anchor_count(A, 1, 2491, 5, 1) == A * cf == SW.anchored_count(A, 1, 2491, 5, 1)
    assert lib.matcha_kway_anchor_count(A + 1, 1, 2491, 5, 1) == -1      # >= 2^63: refused, not truncated
    with pytest.raises(ValueError):
        SW.anchored_count(A + 1, 1, 2491, 5, 1)
    assert lib.matcha_kway_anchor_count(1, 1, 24900, 6, 1) == -1         # C_f alone does not fit
    for A, s, n, k, g in ((-1, 1, 16, 3, 1), (1, 0, 16, 3, 1), (1, 3, 16, 3, 1), (1, 1, 0, 3, 1), (1, 1, 16, 9, 1), (1, 1, 16, 1, 1), (1, 1, 16, 3, 0)):
        assert lib.matcha_kway_anchor_count(A, s, n, k, g) == -1, (A, s, n, k, g)
        with pytest.raises(ValueError):
            SW.anchored_count(A, s, n, k, g)
    assert lib.matcha_kway_anchor_count(3, 7, 16, 8, 1) == 48 and lib.matcha_kway_anchor_count(3, 1, 6, 4, 3) == 0


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    rows = lambda *a: lib.matcha_kway_anchor_rows(*a, None)
    with _lib.launch_log() as log:
        # anchors, A, s, lo, n, k, min_gap, rank0, ranks, count, L, x, flag
        assert rows(p, 4, 1, 1, 16, 3, 1, 0, None, 4, 3, None, p) == -22 and "null output" in err()
        assert rows(p, 4, 1, 1, 16, 3, 1, 0, None, 4, 3, p, None) == -22 and "null output" in err()
        assert rows(None, 4, 1, 1, 16, 3, 1, 0, None, 4, 3, p, p) == -22 and "null anchors" in err()
        assert rows(p, 4, 0, 1, 16, 3, 1, 0, None, 4, 3, p, p) == -22 and "s" in err()                           # s < 1
        assert rows(p, 4, 3, 1, 16, 3, 1, 0, None, 4, 3, p, p) == -22                                             # s > k - 1
        assert rows(p, 4, 1, 1, 16, 3, 1, 0, None, 4, 2, p, p) == -22 and "width" in err()                       # L < k
        assert rows(p, 4, 1, 1, 16, 3, 1, 0, None, 4, 9, p, p) == -22                                             # L > 8
        assert rows(p, 4, 1, 1, 16, 9, 1, 0, None, 4, 8, p, p) == -22
        assert rows(p, 4, 1, 1, 16, 3, 0, 0, None, 4, 3, p, p) == -22
        assert rows(p, -1, 1, 1, 16, 3, 1, 0, None, 0, 3, p, p) == -22
        assert rows(p, 4, 1, 1, 16, 3, 1, 478, None, 4, 3, p, p) == -22 and "outside" in err()                   # 4 * 120 global ranks
        assert rows(p, 4, 1, 1, 16, 3, 1, -1, None, 1, 3, p, p) == -22
        assert rows(p, 1 << 40, 1, 1, 2491, 5, 1, 0, None, 1, 5, p, p) == -22 and "63 bits" in err()             # A C_f >= 2^63
        sb = lib.matcha_segtopk_bytes
        assert sb(4, 0, 10, 100) == 0 and sb(0, 4, 10, 100) == 0 and sb(4, 4, 0, 100) == 0                       # K, A, seg_len < 1
        assert sb(4, 4, 10, 0) == 0 and sb(4, 4, 10, 1 << 31) == 0
        assert sb(1 << 16, 1 << 15, 10, 100) == 0 and sb(1 << 16, (1 << 15) - 1, 10, 100) > 0                    # A K >= 2^31
        need = sb(16, 64, 250, 1000)
        assert need >= 16 * 64 * 16 + 1000 * 12
        assert sb(1, 64, 1 << 62, 1000) >= lib.matcha_topk_bytes(64, 1000) - (1 << 20)
        dims = (16, 64, 250, 1000)
        init, upd, read = lib.matcha_segtopk_init, lib.matcha_segtopk_update, lib.matcha_segtopk_read
        assert init(p, need, 16, 0, 250, 1000, None) == -22 and "K" in err()                                      # K < 1
        assert init(p, need, 1 << 16, 1 << 15, 250, 1000, None) == -22                                            # A K >= 2^31
        assert init(p, need, 16, 64, 0, 1000, None) == -22
        assert init(None, need, *dims, None) == -22
        assert init(p, need - 1, *dims, None) == -22 and "too small" in err()                                     # one byte short
        assert upd(p, need - 1, *dims, 0, p, None, 10, 0, None) == -22 and "too small" in err()
        assert upd(p, need, *dims, 0, p, None, 1001, 0, None) == -22                                              # n > max_chunk
        assert upd(p, need, *dims, 0, None, None, 10, 0, None) == -22 and "null scores" in err()
        assert upd(p, need, *dims, 0, p, None, 10, -1, None) == -22
        assert upd(p, need, *dims, 0, p, None, 10, 16 * 250 - 9, None) == -22 and "outside" in err()              # past the last segment
        assert upd(p, need, *dims, 3, p, None, 10, 3 * 250 - 1, None) == -22 and "outside" in err()               # before the first one
        assert upd(p, need, 16, 0, 250, 1000, 0, p, None, 10, 0, None) == -22
        assert read(p, need - 1, *dims, p, p, p, None) == -22 and "too small" in err()
        assert read(p, need, *dims, None, p, p, None) == -22 and "null output" in err()
        assert read(p, need, *dims, p, p, None, None) == -22 and "null output" in err()
        # no-ops are accepted and launch nothing
        assert rows(p, 4, 1, 1, 16, 3, 1, 0, None, 0, 3, None, None) == 0
        assert rows(None, 0, 1, 1, 16, 3, 1, 0, None, 0, 3, None, None) == 0
        assert upd(p, need, *dims, 0, None, None, 0, 0, None) == 0
        assert upd(p, need, *dims, 3, None, None, 0, 19 * 250, None) == 0
    assert not log.counts
    for kw in (dict(width=2), dict(width=9), dict(rank0=479, count=2), dict(rank0=-1, count=1)):
        with pytest.raises((ValueError, IndexError)):
            SW.anchored_rows(np.arange(1, 5), 1, 16, 3, 1, device="cpu", **kw)
    with pytest.raises(ValueError):
        SW.anchored_rows(np.zeros((4, 3), dtype=np.int64), 1, 16, 3, 1, device="cpu")                            # s > k - 1
    with pytest.raises(_lib.MatchaHipError):
        SW.SegTopK(4, 4, 10, 100, device="cpu")


# ---- the g11 fixture, per anchor ---------------------------------------------------------------------------------------------------
def anchor_ksel(logits):
    """(K_a, gap): K_a in [2, min(16, count - 1)] at the largest gap of the logits sorted downwards, and that gap."""
    s = np.sort(np.asarray(logits, dtype=np.float64))[::-1]
    hi = min(16, len(s) - 1)
    assert hi >= 2
    gaps = s[1:hi] - s[2:hi + 1]                                         # gaps[j]: between the K = j + 2 best and the next
    j = int(np.argmax(gaps))
    return j + 2, float(gaps[j])


def g11_anchor_sets(g):
    """(case index, mode, anchor ids, indices of the fixture rows that contain them) for every single anchor of every case and the
    anchor pairs of the k = 4 and k = 5 cases."""
    num = [int(v) for v in g["num"]]
    starts = np.concatenate([[0], np.cumsum(num)]) + 1
    for i, (c, k, gap) in enumerate(g["cases"]):
        rows, lo = g[f"rows_c{i}"], int(starts[int(c)])
        singles = [(lo + a,) for a in range(num[int(c)])]
        pairs = [(lo + a, lo + b) for a, b in PAIR_OFFSETS] if int(k) >= 4 else []
        for ids in singles + pairs:
            member = np.all([(rows == v).any(axis=1) for v in ids], axis=0)
            for mode in ("table", "adj"):
                yield i, mode, ids, np.flatnonzero(member)


def test_fixture_separates_every_anchors_top_rows():
    g = gold("g11_kway_tiny.npz")
    smallest = {1: np.inf, 2: np.inf}
    seen = {1: 0, 2: 0}
    for i, mode, ids, idx in g11_anchor_sets(g):
        lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
        K, gap = anchor_ksel(lg[idx])
        assert 2 <= K <= min(16, len(idx) - 1)
        rel = gap / np.abs(lg).max()
        assert rel >= 50 * G11_TOL, (i, mode, ids, rel)
        smallest[len(ids)] = min(smallest[len(ids)], rel)
        seen[len(ids)] += 1
    assert seen == {1: 96, 2: 12}
    print("smallest gaps (x max|logit|):", smallest)
    # the pair closer than the gap has no valid candidate in either case
    num = [int(v) for v in g["num"]]
    starts = np.concatenate([[0], np.cumsum(num)]) + 1
    for i, (c, k, gap) in enumerate(g["cases"]):
        if int(k) < 4:
            continue
        lo, n = int(starts[int(c)]), num[int(c)]
        pair = [lo + CLOSE_PAIR[0], lo + CLOSE_PAIR[1]]
        assert not any(SW.anchored_unrank(r, pair, lo, n, int(k), int(gap))[1] for r in range(SW.anchored_count(1, 2, n, int(k), int(gap))))
        rows = g[f"rows_c{i}"]
        assert not ((rows == pair[0]).any(axis=1) & (rows == pair[1]).any(axis=1)).any()
