"""The de novo k-way sweep without a GPU (matcha_amd/sweep.py, the host side of csrc/sweep_rows.hip and csrc/sweep_select.hip): the candidate rule and its ranking
against itertools, the host-only count against math.comb, argument errors refused before any device call, and the fixture's own
consistency (tests/golden/make_golden_kway.py)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from matcha_amd import _lib
from matcha_amd import sweep as SW
from tests.helpers import gold

GRID = [(n, k, g) for n in (1, 2, 6, 7, 12, 16) for k in (2, 3, 4, 5) for g in (1, 2, 3)]
G11_TOL = 1e-4


def brute(lo, n, k, min_gap):
    """The rule restated: ascending k-tuples of [lo, lo + n) with every adjacent difference >= min_gap, in lexicographic order."""
    return [c for c in itertools.combinations(range(lo, lo + n), k) if all(b - a >= min_gap for a, b in zip(c, c[1:]))]


def test_count_and_unrank_match_itertools():
    seen_one = seen_zero = False
    for n, k, g in GRID:
        ref = brute(5, n, k, g)
        assert SW.kway_count(n, k, g) == len(ref), (n, k, g)
        got = [SW.kway_unrank(r, 5, n, k, g) for r in range(len(ref))]
        assert got == ref, (n, k, g)                                     # every rank round-trips
        assert all(a < b for a, b in zip(got, got[1:])), (n, k, g)       # lexicographically increasing
        seen_one |= len(ref) == 1
        seen_zero |= len(ref) == 0
        for bad in (-1, len(ref)):
            with pytest.raises(IndexError):
                SW.kway_unrank(bad, 5, n, k, g)
    assert seen_one and seen_zero
    assert SW.kway_count(7, 3, 3) == 1 and SW.kway_count(6, 3, 3) == 0
    for n, k, g in ((16, 3, 1), (16, 3, 3), (16, 5, 2), (12, 4, 3), (16, 2, 2)):
        m = n - (k - 1) * (g - 1)
        assert SW.kway_count(n, k, g) == math.comb(m, k)


def test_large_ranks_unrank_consistently():
    """Beyond 2^32 nothing can be enumerated: the rank of the unranked row, recomputed from the definition, is the rank asked for."""
    def rank_of(row, lo, n, k, g):
        m = n - (k - 1) * (g - 1)
        y = [x - lo - j * (g - 1) for j, x in enumerate(row)]
        r, prev = 0, -1
        for j, v in enumerate(y):
            for t in range(prev + 1, v):
                r += math.comb(m - 1 - t, k - 1 - j)
            prev = v
        return r
    for n, k, g in ((2491, 4, 1), (2491, 3, 3), (250, 8, 2)):
        total = SW.kway_count(n, k, g)
        for r in (0, 1, total // 3, (1 << 40) % total, total - 2, total - 1):
            row = SW.kway_unrank(r, 1, n, k, g)
            assert all(b - a >= g for a, b in zip(row, row[1:])) and 1 <= row[0] and row[-1] <= n
            assert rank_of(row, 1, n, k, g) == r
    total = SW.kway_count(120000, 4, 1)
    assert SW.kway_unrank(total - 1, 1, 120000, 4, 1) == (119997, 119998, 119999, 120000)
    assert SW.kway_unrank(0, 1, 120000, 4, 1) == (1, 2, 3, 4)


def generate_pair_wise_np(lo, hi, min_dis):
    """denoise_contact.py:67-74 restated in numpy."""
    return np.asarray([(i, j) for i in range(lo, hi) for j in range(i + min_dis, hi)], dtype=np.int64).reshape(-1, 2)


@pytest.mark.parametrize("min_gap", [1, 2])
def test_k2_rows_equal_generate_pair_wise(min_gap):
    for lo, n in ((1, 16), (17, 7), (3, 2), (3, 1)):
        ref = generate_pair_wise_np(lo, lo + n, min_gap)
        got = np.asarray([SW.kway_unrank(r, lo, n, 2, min_gap) for r in range(SW.kway_count(n, 2, min_gap))], dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(got, ref)


def test_library_count_host_only():
    lib = _lib.load()
    for n, k, g in ((250, 5, 1), (2491, 3, 3), (65535, 4, 1), (120000, 4, 1)):
        m = n - (k - 1) * (g - 1)
        assert lib.matcha_kway_count(n, k, g) == math.comb(m, k) == SW.kway_count(n, k, g)
    assert math.comb(120000, 4) > 1 << 62                                # the case whose plain product passes 2^64
    for n, k, g in ((24900, 5, 1), (65535, 5, 1), (250, 1, 1), (250, 9, 1), (250, 3, 0), (0, 3, 1)):
        assert lib.matcha_kway_count(n, k, g) == -1, (n, k, g)
    for n, k, g in GRID:
        assert lib.matcha_kway_count(n, k, g) == len(brute(0, n, k, g))
    with pytest.raises(ValueError):
        SW.kway_count(24900, 5, 1)
    with pytest.raises(ValueError):
        SW.kway_count(250, 9, 1)


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    with _lib.launch_log() as log:
        assert lib.matcha_kway_rows(1, 16, 3, 1, 0, None, 4, 3, None, None) == -22 and "null output" in err()
        assert lib.matcha_kway_rows(1, 16, 3, 1, 0, None, 4, 2, p, None) == -22 and "width" in err()            # L < k
        assert lib.matcha_kway_rows(1, 16, 3, 1, 0, None, 4, 9, p, None) == -22                                   # L > 8
        assert lib.matcha_kway_rows(1, 16, 9, 1, 0, None, 4, 8, p, None) == -22
        assert lib.matcha_kway_rows(1, 16, 3, 0, 0, None, 4, 3, p, None) == -22
        assert lib.matcha_kway_rows(1, 16, 3, 1, 558, None, 4, 3, p, None) == -22 and "outside" in err()          # 560 candidates
        assert lib.matcha_kway_rows(1, 16, 3, 1, -1, None, 1, 3, p, None) == -22
        assert lib.matcha_kway_rows(1, 24900, 5, 1, 0, None, 1, 5, p, None) == -22 and "63 bits" in err()
        assert lib.matcha_topk_bytes(0, 100) == 0 and lib.matcha_topk_bytes(10, 0) == 0 and lib.matcha_topk_bytes(10, 1 << 31) == 0
        need = lib.matcha_topk_bytes(64, 1000)
        assert need >= 64 * 16 + 1000 * 4
        assert lib.matcha_topk_bytes(65536, 1 << 20) >= 65536 * 16
        assert lib.matcha_topk_init(p, need, 0, 1000, None) == -22 and "K" in err()                               # K < 1
        assert lib.matcha_topk_init(None, need, 64, 1000, None) == -22
        assert lib.matcha_topk_init(p, need - 1, 64, 1000, None) == -22 and "too small" in err()
        assert lib.matcha_topk_update(p, need - 1, 64, 1000, p, None, 10, 0, None) == -22 and "too small" in err()
        assert lib.matcha_topk_update(p, need, 64, 1000, p, None, 1001, 0, None) == -22                           # n > max_chunk
        assert lib.matcha_topk_update(p, need, 64, 1000, None, None, 10, 0, None) == -22
        assert lib.matcha_topk_update(p, need, 64, 1000, p, None, 10, -1, None) == -22
        assert lib.matcha_topk_update(p, need, 0, 1000, p, None, 10, 0, None) == -22
        assert lib.matcha_topk_read(p, need - 1, 64, 1000, p, p, p, None) == -22 and "too small" in err()
        assert lib.matcha_topk_read(p, need, 64, 1000, None, p, p, None) == -22 and "null output" in err()
        # no-ops are accepted and launch nothing
        assert lib.matcha_kway_rows(1, 16, 3, 1, 0, None, 0, 3, None, None) == 0
        assert lib.matcha_topk_update(p, need, 64, 1000, None, None, 0, 0, None) == 0
    assert not log.counts
    for kw in (dict(width=2), dict(width=9), dict(rank0=559, count=2), dict(rank0=-1, count=1)):
        with pytest.raises((ValueError, IndexError)):
            SW.kway_rows(1, 16, 3, 1, device="cpu", **kw)


def test_fixture_is_self_consistent():
    g = gold("g11_kway_tiny.npz")
    num = [int(v) for v in g["num"]]
    starts = np.concatenate([[0], np.cumsum(num)]) + 1
    assert [tuple(int(v) for v in c) for c in g["cases"]] == [(0, 3, 1), (2, 4, 2), (1, 5, 3)]
    for i, (c, k, gap) in enumerate(g["cases"]):
        c, k, gap = int(c), int(k), int(gap)
        ref = np.asarray(brute(int(starts[c]), num[c], k, gap), dtype=np.int64)
        assert np.array_equal(g[f"rows_c{i}"], ref) and len(ref) == (560, 715, 56)[i] == SW.kway_count(num[c], k, gap)
        for mode in ("table", "adj"):
            lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
            K = int(g[f"ksel_{mode}_c{i}"])
            assert lg.shape == (len(ref),) and len(np.unique(lg)) == len(lg) and 10 <= K < 50
            s = np.sort(lg)[::-1]
            gaps = s[9:49] - s[10:50]
            assert K == 10 + int(np.argmax(gaps))
            assert s[K - 1] - s[K] >= 100 * G11_TOL * np.abs(lg).max()
