"""Cluster decomposition without a GPU (matcha_amd/sweep.py, the host side of csrc/sweep_rows.hip and csrc/sweep_support.hip): the new entry points and their
refusals before any device call, counts and unranking against the itertools twin (tests/subsets_ref.py), the g16 fixture's consistency,
the fp32 oracle on its rows, and the CLI's line check.  (The host side alone under ASan + UBSan: tests/test_cpu_host_checks.py.)"""
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
from tests import subsets_ref as SR
from tests.helpers import gold, logit_err
from tests.test_cpu_long_rows import golden_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("matcha_cluster_subset_count", "matcha_cluster_subset_rows", "matcha_subset_support_bytes", "matcha_subset_support_init",
       "matcha_subset_support_update", "matcha_subset_support_read")


def test_symbols_in_header_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "matcha_hip.h")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    for name in NEW:
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    rows = lambda *a: lib.matcha_cluster_subset_rows(*a, None)
    with _lib.launch_log() as log:
        # clusters, A, S, m, complement, min_gap, rank0, ranks, count, L, x, flag
        assert rows(p, 4, 9, 3, 0, 1, 0, None, 4, 3, None, p) == -22 and "null output" in err()
        assert rows(p, 4, 9, 3, 0, 1, 0, None, 4, 3, p, None) == -22 and "null output" in err()
        assert rows(None, 4, 9, 3, 0, 1, 0, None, 4, 3, p, p) == -22 and "null clusters" in err()
        assert rows(p, 4, 1, 2, 0, 1, 0, None, 0, 2, p, p) == -22 and "S" in err()                               # S < 2
        assert rows(p, 4, 33, 2, 0, 1, 0, None, 4, 2, p, p) == -22 and "S" in err()                              # S > 32
        assert rows(p, 4, 9, 1, 0, 1, 0, None, 4, 2, p, p) == -22 and "keep" in err()                            # keep: m < 2
        assert rows(p, 4, 9, 0, 1, 1, 0, None, 4, 9, p, p) == -22 and "drop" in err()                            # drop: m < 1
        assert rows(p, 4, 9, 9, 0, 1, 0, None, 4, 9, p, p) == -22 and rows(p, 4, 9, 9, 1, 1, 0, None, 4, 9, p, p) == -22       # m > 8
        assert rows(p, 4, 9, 3, 2, 1, 0, None, 4, 9, p, p) == -22 and "complement" in err()
        assert rows(p, 4, 9, 3, 0, 0, 0, None, 4, 3, p, p) == -22 and "min_gap" in err()
        assert rows(p, 4, 9, 3, 0, 1, 0, None, 4, 2, p, p) == -22 and "width" in err()                           # keep: L < m
        assert rows(p, 4, 9, 3, 0, 1, 0, None, 4, 33, p, p) == -22 and "width" in err()                          # L > 32
        assert rows(p, 4, 9, 2, 1, 1, 0, None, 4, 6, p, p) == -22 and "width" in err()                           # drop: L < S - m
        assert rows(p, -1, 9, 3, 0, 1, 0, None, 0, 3, p, p) == -22
        assert rows(p, 4, 9, 1, 1, 1, 34, None, 4, 9, p, p) == -22 and "outside" in err()                        # 4 * 9 global ranks
        assert rows(p, 4, 9, 1, 1, 1, -1, None, 1, 9, p, p) == -22 and "outside" in err()
        assert rows(p, 4, 9, 1, 1, 1, 0, None, -1, 9, p, p) == -22
        assert rows(p, (1 << 63) - 1, 32, 8, 0, 1, 0, None, 1, 8, p, p) == -22 and "63 bits" in err()            # A C_m >= 2^63
        # no-ops are accepted and launch nothing
        assert rows(p, 4, 9, 3, 0, 1, 0, None, 0, 3, None, None) == 0
        assert rows(p, 4, 9, 3, 0, 1, 4 * 84, None, 0, 3, None, None) == 0
        assert rows(None, 0, 9, 3, 0, 1, 0, None, 0, 3, None, None) == 0
        assert rows(p, 4, 9, 3, 1, 1, 0, p, 0, 6, None, None) == 0                                               # an empty rank list
        # the support state
        need = lib.matcha_subset_support_bytes(4, 9, 3, 1.0)
        assert need == 256 + 2 * 512
        for bad in ((0, 9, 3, 1.0), (4, 1, 3, 1.0), (4, 33, 3, 1.0), (4, 9, 0, 1.0), (4, 9, 9, 1.0), (4, 9, 3, 0.0), (4, 9, 3, float("nan")),
                    (4, 9, 3, 3e6), ((1 << 40) + 1, 9, 3, 1.0)):
            assert lib.matcha_subset_support_bytes(*bad) == 0, bad
        assert lib.matcha_subset_support_init(None, need, 4, 9, 3, 1.0, None) == -22 and "null state" in err()
        assert lib.matcha_subset_support_init(p, need - 1, 4, 9, 3, 1.0, None) == -22 and "too small" in err()
        assert lib.matcha_subset_support_init(p, need, 4, 33, 3, 1.0, None) == -22 and "S" in err()
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, None, None, 4, 0, None) == -22 and "null value" in err()
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, p, None, 4, 4 * 84 - 3, None) == -22 and "outside" in err()
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, p, None, 1, -1, None) == -22 and "outside" in err()
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, p, None, -1, 0, None) == -22
        assert lib.matcha_subset_support_update(p, need - 8, 4, 9, 3, 1.0, p, None, 4, 0, None) == -22 and "too small" in err()
        assert lib.matcha_subset_support_read(p, need, 4, 9, 3, 1.0, None, None, None, None) == -22 and "null output" in err()
        assert lib.matcha_subset_support_read(None, need, 4, 9, 3, 1.0, p, p, p, None) == -22 and "null state" in err()
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, None, None, 0, 0, None) == 0              # n = 0: nothing launched
        assert lib.matcha_subset_support_update(p, need, 4, 9, 3, 1.0, p, p, 0, 4 * 84, None) == 0
    assert not log.counts
    nine = [list(range(1, 10))] * 4
    for kw in (dict(width=2), dict(width=33), dict(rank0=4 * 84 - 1, count=2), dict(rank0=-1, count=1), dict(min_gap=0)):
        with pytest.raises((ValueError, IndexError)):
            SW.subset_rows(nine, 3, 0, device="cpu", **kw)
    with pytest.raises(ValueError):
        SW.subset_rows(nine, 2, 1, width=6, device="cpu")                # drop: S - m = 7
    for m, comp in ((1, 0), (9, 0), (0, 1), (9, 1), (3, 2)):
        with pytest.raises(ValueError):
            SW.subset_rows(nine, m, comp, device="cpu")
    with pytest.raises(ValueError, match="33 ids"):
        SW.subset_rows([list(range(1, 34))], 2, device="cpu")
    with pytest.raises(_lib.MatchaHipError):
        SW.subset_rows([list(range(1, 33))], 2, device="cpu")            # 32 ids and every argument fine: no CPU fallback
    with pytest.raises(_lib.MatchaHipError):
        SW.SubsetSupport(4, 9, 3, device="cpu")
    # completion's own limit is what it was
    assert SW.MAX_CLUSTER == 31
    with pytest.raises(ValueError, match="32 ids"):
        SW.completion_rows([list(range(1, 33))], 1, 16, 1, 1, device="cpu")


def test_counts_match_the_twin_and_the_library():
    lib = _lib.load()
    for A in (0, 1, 5):
        for S in (2, 3, 8, 9, 31, 32):
            for m in range(1, 9):
                for comp in (0, 1):
                    if m == 1 and not comp:
                        continue
                    want = SR.count(A, S, m)
                    assert lib.matcha_cluster_subset_count(A, S, m, comp) == want == SW.subset_count(A, S, m, comp), (A, S, m, comp)
    assert SW.subset_count(1, 32, 8) == 10518300 == math.comb(32, 8) and SW.subset_count(7, 2, 3) == 0
    assert len(SR.choices(9, 3)) == 84 and len(SR.choices(32, 2)) == 496
    cm = math.comb(32, 8)
    A = ((1 << 63) - 1) // cm
    assert lib.matcha_cluster_subset_count(A, 32, 8, 0) == A * cm == SW.subset_count(A, 32, 8)
    assert lib.matcha_cluster_subset_count(A + 1, 32, 8, 0) == -1          # >= 2^63: refused, not truncated
    with pytest.raises(ValueError):
        SW.subset_count(A + 1, 32, 8)
    for A, S, m, comp in ((-1, 9, 3, 0), (1, 1, 2, 0), (1, 33, 2, 0), (1, 9, 1, 0), (1, 9, 0, 1), (1, 9, 9, 0), (1, 9, 9, 1), (1, 9, 3, 2), (1, 9, 3, -1)):
        assert lib.matcha_cluster_subset_count(A, S, m, comp) == -1, (A, S, m, comp)
        with pytest.raises(ValueError):
            SW.subset_count(A, S, m, comp)


def g16_case(g, i):
    """(clusters as id lists, m, complement, min_gap, W) of fixture case i."""
    mode, m, gap, W, sizes = SR.G16_CASES[i]
    clusters = [SR.leading_ids(r) for r in g[f"clusters_c{i}"].astype(np.int64)]
    assert [len(cl) for cl in clusters] == list(sizes)
    return clusters, m, int(mode == "drop"), gap, W


def test_unrank_matches_the_twin_on_every_rank_of_the_fixture_cases():
    g = gold("g16_subsets_tiny.npz")
    for i in range(len(SR.G16_CASES)):
        clusters, m, comp, gap, W = g16_case(g, i)
        for cl in clusters:
            ref = SR.candidates(cl, len(cl), m, comp, gap)
            assert len(ref) == SW.subset_count(1, len(cl), m, comp)
            assert [SW.subset_unrank(r, cl, m, comp, gap) for r in range(len(ref))] == ref, (i, cl)
            for bad in (-1, len(ref)):
                with pytest.raises(IndexError):
                    SW.subset_unrank(bad, cl, m, comp, gap)
    # the edges of the rule: the order of the choices, a repeated id, the gap, a descending cluster, a choice past the ids, ids behind a zero
    assert [SW.subset_unrank(r, [4, 9, 20], 2)[0] for r in range(3)] == [(4, 9), (4, 20), (9, 20)]
    assert [SW.subset_unrank(r, [4, 9, 20], 1, 1)[0] for r in range(3)] == [(9, 20), (4, 20), (4, 9)]
    assert SW.subset_unrank(0, [4, 4, 9], 2) == ((4, 4), False) and SW.subset_unrank(1, [4, 4, 9], 2) == ((4, 9), True)
    assert SW.subset_unrank(0, [4, 6, 9], 2, 0, 3) == ((4, 6), False) and SW.subset_unrank(1, [4, 6, 9], 2, 0, 3) == ((4, 9), True)
    assert SW.subset_unrank(1, [4, 6, 9], 1, 1, 3) == ((4, 9), True) and SW.subset_unrank(2, [4, 6, 9], 1, 1, 3) == ((4, 6), False)
    assert SW.subset_unrank(2, [9, 4, 20], 2) == ((4, 20), False) == SR.candidates([9, 4, 20], 3, 2, 0, 1)[2]          # the CLUSTER descends
    assert SW.subset_unrank(1, [4, 9, 0, 0], 2) == ((), False) and SW.subset_unrank(0, [4, 9, 0, 0], 2) == ((4, 9), True)
    assert SW.subset_unrank(0, [4, 9, 0, 30], 1, 1) == ((9,), False) == SR.candidates([4, 9, 0, 30], 4, 1, 1, 1)[0]    # fewer than 2 ids
    assert SW.subset_unrank(3, [4, 9, 0, 30], 1, 1) == ((), False)                                                      # position 3 holds no id
    assert SW.subset_unrank(0, [4, 9, 12, 0], 1, 1) == ((9, 12), True)


def test_fixture_is_self_consistent():
    g = gold("g16_subsets_tiny.npz")
    assert [int(v) for v in g["num"]] == [16, 16, 16, 16] and int(g["seed_base"]) == SR.G16_SEED
    n_rows, with_invalid = 0, 0
    for i in range(len(SR.G16_CASES)):
        clusters, m, comp, gap, W = g16_case(g, i)
        assert clusters == SR.g16_clusters(i)
        rows, bad, off = SR.g16_rows(i)
        assert np.array_equal(g[f"rows_c{i}"].astype(np.int64), rows) and np.array_equal(g[f"valid_c{i}"], ~bad)
        assert np.array_equal(g[f"offsets_c{i}"], off) and rows.shape[1] == W
        n_rows += len(rows)
        with_invalid += bool(bad.any())
        for mode in ("table", "adj"):
            lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
            assert lg.shape == (len(rows),) and g[f"logit_{mode}_c{i}"].dtype == np.float32
            assert (f"full_{mode}_c{i}" in g.files) == bool(comp)
            if comp:
                assert g[f"full_{mode}_c{i}"].shape == (len(clusters),)
            sup = g[f"support_{mode}_c{i}"]
            assert sup.dtype == np.float64 and sup.shape == (len(clusters), max(len(c) for c in clusters))
            for a, cl in enumerate(clusters):
                seg = slice(int(off[a]), int(off[a + 1]))
                assert off[a + 1] - off[a] == math.comb(len(cl), m)
                valid = lg[seg][~bad[seg]]
                assert len(valid) >= 3
                K, gap_abs = CR.k_sel(valid)
                assert K == int(g[f"ksel_{mode}_c{i}"][a]) and 2 <= K <= min(8, len(valid) - 1)
                assert gap_abs >= 50 * SR.G16_TOL * np.abs(valid).max(), (i, mode, a)
                # the per-locus sums are what the logits say, and every valid row is counted once per chosen position
                p = 1.0 / (1.0 + np.exp(-lg[seg]))
                want = np.zeros(sup.shape[1])
                for r, ch in enumerate(SR.choices(len(cl), m)):
                    if not bad[seg][r]:
                        want[list(ch)] += p[r]
                assert np.allclose(sup[a], want, rtol=1e-12, atol=0) and abs(sup[a].sum() - m * p[~bad[seg]].sum()) <= 1e-9 * m * len(p)
    assert 3000 <= n_rows <= 4000 and with_invalid == 1                  # case 2 (min_gap 2) holds the invalid rows
    assert [int(g["valid_c2"][g["offsets_c2"][a]:g["offsets_c2"][a + 1]].sum()) for a in range(3)] == [28, 225, 806]


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_oracle_reproduces_the_reference_on_the_fixture(mode):
    """The bound, 1e-5 logit_err, is two to three times the fp32 oracle's own rounding on these 3 492 rows (element-wise, against a
    floor of 5 % of the largest logit), and the oracle's rounding follows the CPU's BLAS path.  Measured worst case (always the adj
    model, case 0 or 1): 3.3e-6 with the AVX-512 path the fixture was made with; 8.2e-6 with MKL held to AVX2, 6.7e-6 to SSE4.2, 9.4e-6
    in MKL's compatibility mode; 1.01e-5 on the CPU of one GPU host (case 0), which misses the bound by 1.5 %.  The table model stays
    below 6.4e-6 on all of them.  tests/test_cpu_complete.py's twin of this test has the same sensitivity (1.15e-5 in compatibility mode)."""
    g = gold("g16_subsets_tiny.npz")
    P, fe = golden_oracle(mode)
    with torch.no_grad():
        for i in range(len(SR.G16_CASES)):
            clusters, m, comp, gap, W = g16_case(g, i)
            x = torch.from_numpy(g[f"rows_c{i}"].astype(np.int64))
            assert x.shape[1] == W
            lg, _ = O.classifier_forward(P, fe, x, random_chrom=0)
            lg, ref = lg.numpy().reshape(-1).astype(np.float64), g[f"logit_{mode}_c{i}"].astype(np.float64)
            e = logit_err(lg, ref)
            print(f"{mode} case {i}: logit_err {e:.2e}")
            assert e <= 1e-5, (mode, i, e)
            off, valid = g[f"offsets_c{i}"], g[f"valid_c{i}"]
            for a in range(len(clusters)):                               # the oracle's top K_a of every cluster is the reference's
                ok = np.flatnonzero(valid[off[a]:off[a + 1]]) + int(off[a])
                K = int(g[f"ksel_{mode}_c{i}"][a])
                assert set(ok[np.argsort(-lg[ok])[:K]].tolist()) == set(ok[np.argsort(-ref[ok])[:K]].tolist()), (mode, i, a)
            if comp:
                whole = torch.from_numpy(SR.padded(clusters, W))
                fl, _ = O.classifier_forward(P, fe, whole, random_chrom=0)
                e = logit_err(fl.numpy().reshape(-1).astype(np.float64), g[f"full_{mode}_c{i}"].astype(np.float64))
                assert e <= 1e-5, (mode, i, e)


def test_twin_support_identities():
    """The integer restatement the GPU planes are compared with: counts and sums add up per row, skips and rejects land in the counters,
    and the state does not depend on how the ranks are cut."""
    A, S, m = 3, 5, 2
    cm = math.comb(S, m)
    rng = np.random.default_rng(4)
    v = rng.random(A * cm).astype(np.float32)
    v[[3, 11]] = [np.nan, 1.5]
    skip = rng.random(A * cm) < 0.2
    skip[[3]] = False
    total, cnt, counters = SR.support(A, S, m, v, skip, 0)
    live = ~skip & (v >= 0) & (v <= 1)
    assert counters == [int(live.sum()), 2 - int(skip[11])]
    for a in range(A):
        seg = slice(a * cm, (a + 1) * cm)
        assert cnt[a].sum() == m * live[seg].sum() and total[a].sum() == m * sum(SR.quantum(q) for q in v[seg][live[seg]])
    state = None
    for lo, hi in ((17, 30), (0, 5), (5, 17)):
        state = SR.support(A, S, m, v[lo:hi], skip[lo:hi], lo, state=state)
    assert np.array_equal(state[0], total) and np.array_equal(state[1], cnt) and state[2] == counters
    assert SR.quantum(0.5) == 1 << 31 and SR.quantum(1.0) == 1 << 32 and SR.quantum(np.float32(1e-10)) == 0


def _write_lines(path, lines):
    with open(path, "w") as f:
        for loci in lines:
            f.write("\t".join("chr1:%d" % (b * 100 + 7) for b in loci) + "\n")


def test_cli_line_check(tmp_path):
    bin2node = {"chr1:%d" % (b * 100): b + 1 for b in range(64)}
    path = os.path.join(tmp_path, "clusters.txt")
    ok = [[5, 9], list(range(32)), [9, 3, 3, 20], list(range(20)) + list(range(20))]
    _write_lines(path, ok)
    clusters, lines = PR.parse_cluster_file(path, bin2node, ["chr1"], 100, least=2, most=32)
    assert clusters == [[6, 10], list(range(1, 33)), [4, 10, 21], list(range(1, 21))] and lines == [1, 2, 3, 4]
    with open(path, "a") as f:
        f.write("\n" + "chrX:5\tchrY:900\n")                             # an empty line and one without a known chromosome: dropped
    clusters, lines = PR.parse_cluster_file(path, bin2node, ["chr1"], 100, least=2, most=32)
    assert len(clusters) == 4 and lines == [1, 2, 3, 4]
    _write_lines(path, ok + [list(range(33)), [1]])
    with pytest.raises(ValueError, match=r"line 5 has 33 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100, least=2, most=32)
    _write_lines(path, ok + [[7, 7]])
    with pytest.raises(ValueError, match=r"line 5 has 1 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100, least=2, most=32)
    # complete's own bounds are what they were
    _write_lines(path, [[5], list(range(31))])
    assert [len(c) for c in PR.parse_cluster_file(path, bin2node, ["chr1"], 100)[0]] == [1, 31]
    _write_lines(path, [[5], list(range(32))])
    with pytest.raises(ValueError, match=r"line 2 has 32 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
