"""Cluster completion without a GPU (matcha_amd/sweep.py, csrc/sweep_rows.hip's host side): the two entry points and their
refusals before any device call, counts and unranking against the itertools twin (tests/complete_ref.py) and against the anchored
sweep's unranking, the g15 fixture's consistency, the fp32 oracle on its rows, and the CLI's line check."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR
from matcha_amd import sweep as SW
from oracle import hypersagnn as O
from tests import complete_ref as CR
from tests.helpers import gold, logit_err
from tests.test_cpu_long_rows import golden_oracle

GRID = [(A, S, n, f, g) for A in (0, 1, 5) for S in (1, 8, 9, 31) for n in (1, 7, 12) for f in (1, 2, 3, 8) for g in (1, 2, 3)]


def test_symbols_in_header_signatures_and_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "matcha_hip.h")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("matcha_kway_complete_count", "matcha_kway_complete_rows"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    rows = lambda *a: lib.matcha_kway_complete_rows(*a, None)
    with _lib.launch_log() as log:
        # clusters, A, S, lo, n, f, min_gap, rank0, ranks, count, L, x, flag
        assert rows(p, 4, 9, 1, 16, 1, 1, 0, None, 4, 10, None, p) == -22 and "null output" in err()
        assert rows(p, 4, 9, 1, 16, 1, 1, 0, None, 4, 10, p, None) == -22 and "null output" in err()
        assert rows(None, 4, 9, 1, 16, 1, 1, 0, None, 4, 10, p, p) == -22 and "null clusters" in err()
        assert rows(p, 4, 0, 1, 16, 1, 1, 0, None, 4, 10, p, p) == -22 and "S" in err()                          # S < 1
        assert rows(p, 4, 32, 1, 16, 1, 1, 0, None, 4, 32, p, p) == -22 and "S" in err()                         # S > 31
        assert rows(p, 4, 9, 1, 16, 0, 1, 0, None, 4, 10, p, p) == -22                                            # f < 1
        assert rows(p, 4, 9, 1, 16, 9, 1, 0, None, 4, 18, p, p) == -22                                            # f > 8
        assert rows(p, 4, 9, 1, 16, 2, 1, 0, None, 4, 10, p, p) == -22 and "width" in err()                      # L < S + f
        assert rows(p, 4, 31, 1, 16, 1, 1, 0, None, 4, 33, p, p) == -22 and "width" in err()                     # L > 32
        assert rows(p, 4, 30, 1, 16, 3, 1, 0, None, 4, 32, p, p) == -22 and "width" in err()                     # S + f > 32
        assert rows(p, 4, 9, 1, 16, 1, 0, 0, None, 4, 10, p, p) == -22                                            # min_gap < 1
        assert rows(p, 4, 9, 1, 0, 1, 1, 0, None, 0, 10, p, p) == -22                                             # n < 1
        assert rows(p, -1, 9, 1, 16, 1, 1, 0, None, 0, 10, p, p) == -22
        assert rows(p, 4, 9, -1, 16, 1, 1, 0, None, 4, 10, p, p) == -22 and "lo" in err()
        assert rows(p, 4, 9, 1, 16, 1, 1, 62, None, 4, 10, p, p) == -22 and "outside" in err()                   # 4 * 16 global ranks
        assert rows(p, 4, 9, 1, 16, 1, 1, -1, None, 1, 10, p, p) == -22 and "outside" in err()
        assert rows(p, 4, 9, 1, 16, 1, 1, 0, None, -1, 10, p, p) == -22
        assert rows(p, 1 << 40, 9, 1, 2491, 4, 1, 0, None, 1, 13, p, p) == -22 and "63 bits" in err()            # A C_f >= 2^63
        # no-ops are accepted and launch nothing
        assert rows(p, 4, 9, 1, 16, 1, 1, 0, None, 0, 10, None, None) == 0
        assert rows(p, 4, 9, 1, 16, 1, 1, 64, None, 0, 10, None, None) == 0
        assert rows(None, 0, 9, 1, 16, 1, 1, 0, None, 0, 10, None, None) == 0
        assert rows(p, 4, 9, 1, 16, 1, 1, 0, p, 0, 10, None, None) == 0                                           # an empty rank list
    assert not log.counts
    for kw in (dict(width=9), dict(width=33), dict(rank0=63, count=2), dict(rank0=-1, count=1)):
        with pytest.raises((ValueError, IndexError)):
            SW.completion_rows([list(range(1, 10))] * 4, 1, 16, 1, 1, device="cpu", **kw)
    for free in (0, 9):
        with pytest.raises(ValueError):
            SW.completion_rows([[1, 2]], 1, 16, free, 1, device="cpu")
    with pytest.raises(ValueError, match="32 ids"):
        SW.completion_rows([list(range(1, 33))], 1, 16, 1, 1, device="cpu")
    with pytest.raises(_lib.MatchaHipError):
        SW.completion_rows([[1, 2]], 1, 16, 1, 1, device="cpu")         # every argument is fine: no CPU fallback


def test_counts_match_the_twin_and_the_library():
    lib = _lib.load()
    for A, S, n, f, g in GRID:
        want = CR.count(A, n, f, g)
        assert lib.matcha_kway_complete_count(A, S, n, f, g) == want == SW.completion_count(A, S, n, f, g), (A, S, n, f, g)
    assert SW.completion_count(3, 31, 16, 1, 1) == 48 and SW.completion_count(3, 1, 6, 3, 3) == 0
    cf = math.comb(2491, 4)
    assert cf > 1 << 40
    A = ((1 << 63) - 1) // cf
    assert lib.matcha_kway_complete_count(A, 12, 2491, 4, 1) == A * cf == SW.completion_count(A, 12, 2491, 4, 1)
    assert lib.matcha_kway_complete_count(A + 1, 12, 2491, 4, 1) == -1     # >= 2^63: refused, not truncated
    with pytest.raises(ValueError):
        SW.completion_count(A + 1, 12, 2491, 4, 1)
    assert lib.matcha_kway_complete_count(1, 12, 24900, 5, 1) == -1        # C_f alone does not fit
    for A, S, n, f, g in ((-1, 9, 16, 1, 1), (1, 0, 16, 1, 1), (1, 32, 16, 1, 1), (1, 9, 0, 1, 1), (1, 9, 16, 0, 1), (1, 9, 16, 9, 1), (1, 9, 16, 1, 0)):
        assert lib.matcha_kway_complete_count(A, S, n, f, g) == -1, (A, S, n, f, g)
        with pytest.raises(ValueError):
            SW.completion_count(A, S, n, f, g)


def g15_case(g, i):
    """(clusters as id lists, lo, n, free, min_gap, W) of fixture case i."""
    c, free, gap, W, sizes = CR.G15_CASES[i]
    num = [int(v) for v in g["num"]]
    lo = int(np.concatenate([[0], np.cumsum(num)])[c]) + 1
    clusters = [CR.leading_ids(r) for r in g[f"clusters_c{i}"].astype(np.int64)]
    assert [len(cl) for cl in clusters] == list(sizes)
    return clusters, lo, num[c], free, gap, W


def test_unrank_matches_the_twin_on_every_rank_of_the_fixture_cases():
    g = gold("g15_complete_tiny.npz")
    for i in range(len(CR.G15_CASES)):
        clusters, lo, n, free, gap, W = g15_case(g, i)
        for cl in clusters:
            ref = CR.candidates(cl, lo, n, free, gap)
            assert len(ref) == SW.completion_count(1, len(cl), n, free, gap)
            assert [SW.completion_unrank(r, cl, lo, n, free, gap) for r in range(len(ref))] == ref, (i, cl)
            for bad in (-1, len(ref)):
                with pytest.raises(IndexError):
                    SW.completion_unrank(bad, cl, lo, n, free, gap)
    # the edges of the rule: a free id on a cluster id, a repeated id, a descending cluster, an empty one, ids behind a zero
    assert SW.completion_unrank(3, [4, 9], 1, 12, 1, 1) == ((4, 4, 9), False)
    assert SW.completion_unrank(4, [4, 9], 1, 12, 1, 1) == ((4, 5, 9), True) and SW.completion_unrank(4, [4, 9], 1, 12, 1, 2) == ((4, 5, 9), False)
    assert SW.completion_unrank(0, [4, 4], 1, 12, 1, 1) == ((1, 4, 4), False)
    assert SW.completion_unrank(0, [9, 4], 1, 12, 1, 1) == ((9, 4, 1), False) == CR.candidates([9, 4], 1, 12, 1, 1)[0]
    assert SW.completion_unrank(2, [], 1, 12, 2, 2) == ((1, 5), False) == CR.candidates([0, 0], 1, 12, 2, 2)[2]
    assert SW.completion_unrank(0, [20, 0, 30], 1, 12, 1, 1) == ((1, 20), True) == CR.candidates([20, 0, 30], 1, 12, 1, 1)[0]


def test_unrank_agrees_with_the_anchored_unranking():
    """Uniform clusters with S + f <= 8: the anchored sweep's candidates, rank for rank."""
    for lo, n in ((1, 12), (5, 16)):
        for s in (1, 2, 5, 7):
            for f in [f for f in range(1, 9 - s) if f <= 3 or (n == 12 and s + f == 8)]:      # the widest free parts on the small region only
                for g in (1, 2, 3):
                    for cluster in ([lo + 2 + 3 * j for j in range(s)], [lo + n + 3 + 3 * j for j in range(s)], [lo + 3, lo + 3 + g - 1][:s]):
                        if len(cluster) != s:
                            continue
                        cf = SW.anchored_count(1, s, n, s + f, g)
                        assert cf == SW.completion_count(1, s, n, f, g)
                        for r in range(cf):
                            assert SW.completion_unrank(r, cluster, lo, n, f, g) == SW.anchored_unrank(r, cluster, lo, n, s + f, g), (lo, n, s, f, g, r)


def test_fixture_is_self_consistent():
    g = gold("g15_complete_tiny.npz")
    assert [int(v) for v in g["num"]] == [16, 16, 16, 16] and int(g["seed_base"]) == CR.G15_SEED
    for i in range(len(CR.G15_CASES)):
        clusters, lo, n, free, gap, W = g15_case(g, i)
        assert clusters == CR.g15_clusters(i)
        rows, bad = CR.table(clusters, lo, n, free, gap, W)
        assert np.array_equal(g[f"rows_c{i}"].astype(np.int64), rows) and np.array_equal(g[f"valid_c{i}"], ~bad)
        cf = len(rows) // len(clusters)
        for mode in ("table", "adj"):
            lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
            assert lg.shape == (len(rows),) and g[f"logit_{mode}_c{i}"].dtype == np.float32
            for a in range(len(clusters)):
                seg = slice(a * cf, (a + 1) * cf)
                assert len(np.unique(lg[seg])) == cf
                valid = lg[seg][~bad[seg]]
                assert 3 <= len(valid) <= 120
                K, gap_abs = CR.k_sel(valid)
                assert K == int(g[f"ksel_{mode}_c{i}"][a]) and 2 <= K <= min(8, len(valid) - 1)
                assert gap_abs >= 50 * CR.G15_TOL * np.abs(valid).max(), (i, mode, a)


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_oracle_reproduces_the_reference_on_the_fixture(mode):
    g = gold("g15_complete_tiny.npz")
    P, fe = golden_oracle(mode)
    with torch.no_grad():
        for i in range(len(CR.G15_CASES)):
            clusters, lo, n, free, gap, W = g15_case(g, i)
            x = torch.from_numpy(g[f"rows_c{i}"].astype(np.int64))
            assert x.shape[1] == W
            lg, _ = O.classifier_forward(P, fe, x, random_chrom=0)
            lg, ref = lg.numpy().reshape(-1).astype(np.float64), g[f"logit_{mode}_c{i}"].astype(np.float64)
            e = logit_err(lg, ref)
            print(f"{mode} case {i}: logit_err {e:.2e}")
            assert e <= 1e-5, (mode, i, e)
            cf = len(ref) // len(clusters)
            for a in range(len(clusters)):                               # the oracle's top K_a of every cluster is the reference's
                ok = np.flatnonzero(g[f"valid_c{i}"][a * cf:(a + 1) * cf]) + a * cf
                K = int(g[f"ksel_{mode}_c{i}"][a])
                assert set(ok[np.argsort(-lg[ok])[:K]].tolist()) == set(ok[np.argsort(-ref[ok])[:K]].tolist()), (mode, i, a)


def _write_lines(path, lines):
    with open(path, "w") as f:
        for loci in lines:
            f.write("\t".join("chr1:%d" % (b * 100 + 7) for b in loci) + "\n")


def test_cli_line_check(tmp_path):
    bin2node = {"chr1:%d" % (b * 100): b + 1 for b in range(64)}
    path = os.path.join(tmp_path, "clusters.txt")
    ok = [[5], list(range(31)), [9, 3, 3, 20], list(range(20)) + list(range(20))]
    _write_lines(path, ok)
    clusters, lines = PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
    assert clusters == [[6], list(range(1, 32)), [4, 10, 21], list(range(1, 21))] and lines == [1, 2, 3, 4]
    with open(path, "a") as f:
        f.write("\n" + "chrX:5\tchrY:900\n")                             # an empty line and one without a known chromosome: dropped
    _write_lines(path + "2", [[1, 2]])
    clusters, lines = PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
    assert len(clusters) == 4 and lines == [1, 2, 3, 4]
    _write_lines(path, ok + [list(range(32)), [1]])
    with pytest.raises(ValueError, match=r"line 5 has 32 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
    with pytest.raises(ValueError, match=r"line 2 has 31 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100, free=2)
    _write_lines(path, [[1, 2], list(range(30))])
    assert [len(c) for c in PR.parse_cluster_file(path, bin2node, ["chr1"], 100, free=2)[0]] == [2, 30]
