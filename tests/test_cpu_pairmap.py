"""Pair maps without a GPU: the numpy restatement (tests/pairmap_ref.py) against the reference's proba2matrix and
against plain numpy, the refusals of the C ABI (the library loads without a device and refuses before any device call), and the
conditions the GPU test against the reference's logits rests on, asserted on the reference's own numbers."""
import ctypes as C
import itertools

import numpy as np
import pytest

from matcha_amd import _lib
from matcha_amd import predict as PR
from matcha_amd import sweep as SW
from matcha_amd import synth
from tests.helpers import gold
from tests.pairmap_ref import SCALE, golden_cut, pairmap_ref

G11_TOL = 1e-4                   # the device forward against the reference's CPU logits (tests/test_hip_kway.py)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_equals_proba2matrix_for_duplicate_free_pairs():
    rng = np.random.default_rng(0)
    lo, n = 11, 23
    pairs = np.asarray([(i, j) for i in range(lo, lo + n) for j in range(i + 2, lo + n)], dtype=np.int64)
    pairs = pairs[rng.permutation(len(pairs))]
    assert pairs.min() == lo and pairs.max() == lo + n - 1               # proba2matrix sizes its matrix by the ids it sees
    p = rng.random(len(pairs)).astype(np.float32)
    ref = PR.proba2matrix(pairs, None, p, intra=True)
    got = pairmap_ref(pairs, p, (lo, n), (lo, n))
    hit = got["count"] > 0
    assert got["count"].max() == 1 and hit.sum() == 2 * len(pairs) and not ref[~hit].any()
    assert np.array_equal(np.where(hit, got["max"], np.float32(0)).view(np.uint32), ref.view(np.uint32))
    assert np.abs(got["sum"] / SCALE - ref.astype(np.float64)).max() <= 2.0 ** -33
    assert got["n_rows"] == len(pairs) and got["n_rejected"] == 0
    # rectangular: rows from one window, columns from a disjoint one, both orders of the two ids inside a pair
    (lo_r, n_r), (lo_c, n_c) = (3, 5), (40, 9)
    rect = np.asarray([(a, b) for a in range(lo_r, lo_r + n_r) for b in range(lo_c, lo_c + n_c)], dtype=np.int64)
    rect = rect[rng.permutation(len(rect))]
    p = rng.random(len(rect)).astype(np.float32)
    ref = PR.proba2matrix(rect, None, p, intra=False)
    flip = rng.random(len(rect)) < 0.5
    mixed = np.where(flip[:, None], rect[:, ::-1], rect)
    for x in (rect, mixed):
        got = pairmap_ref(x, p, (lo_r, n_r), (lo_c, n_c))
        assert (got["count"] == 1).all()
        assert np.array_equal(got["max"].view(np.uint32), ref.view(np.uint32))
        assert np.abs(got["sum"] / SCALE - ref.astype(np.float64)).max() <= 2.0 ** -33


def test_restatement_accumulates_where_proba2matrix_overwrites():
    rng = np.random.default_rng(1)
    lo, n = 1, 12
    rows = np.asarray(list(itertools.combinations(range(lo, lo + n), 3)), dtype=np.int64)
    p = (rng.random(len(rows)) * 0.75 + 0.25).astype(np.float32)         # >= 2^-8: the fixed-point conversion is exact
    got = pairmap_ref(rows, p, (lo, n), (lo, n))
    q = np.rint(p.astype(np.float64) * SCALE).astype(np.int64)
    assert np.array_equal(q / SCALE, p.astype(np.float64))
    want = np.zeros((n, n), dtype=np.int64)
    cnt = np.zeros((n, n), dtype=np.int64)
    for ci, cj in ((0, 1), (0, 2), (1, 2)):
        np.add.at(want, (rows[:, ci] - lo, rows[:, cj] - lo), q)
        np.add.at(cnt, (rows[:, ci] - lo, rows[:, cj] - lo), 1)
    assert np.array_equal(got["sum"], want + want.T) and np.array_equal(got["count"], cnt + cnt.T)
    assert (got["count"][~np.eye(n, dtype=bool)] == n - 2).all()         # every pair lies in n - 2 triples
    # the reference's fancy-index += keeps the LAST write of a repeated cell: a different matrix (the quirk the restatement drops)
    ref = PR.proba2matrix(rows, None, p, intra=True)
    assert np.abs(ref.astype(np.float64) - got["sum"] / SCALE).max() > 1.0
    # a row with a repeated id adds once per pair of POSITIONS; ids outside the region, zeros and rejected values add nothing
    x = np.asarray([[5, 5, 9], [5, 0, 9], [5, 9, 99], [9, 5, 0], [5, 9, 0], [5, 9, 0], [5, 9, 0], [5, 9, 0]], dtype=np.int64)
    v = np.asarray([0.5, 0.25, 1.0, 0.125, np.nan, -1.0, 1.5, np.inf], dtype=np.float32)
    got = pairmap_ref(x, v, (lo, n), (lo, n))
    assert got["count"][4, 8] == got["count"][8, 4] == 5 and got["count"].sum() == 10
    assert got["sum"][4, 8] == int((0.5 * 2 + 0.25 + 1.0 + 0.125) * SCALE) and got["max"][4, 8] == 1.0 and got["count_ge"][4, 8] == 3
    assert got["n_rows"] == 4 and got["n_rejected"] == 4


# ---- the C ABI refuses without a device --------------------------------------------------------------------------------------------
def test_abi_refusals_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    B = lib.matcha_pairmap_bytes
    ok = (1, 7, 1, 7, 15, 1.0, 0.5)
    with _lib.launch_log() as log:
        need = B(*ok)
        assert need == 256 + 3 * 512 + 256                               # header, three int64 planes of 49 cells, one uint32 plane
        assert B(1, 7, 1, 7, 8, 1.0, 0.5) == 512 and B(1, 5, 40, 9, 1, 1.0, 0.5) == 256 + 512
        assert B(1, 0, 1, 0, 15, 1.0, 0.5) == 0 and B(1, 7, 20, 0, 15, 1.0, 0.5) == 0 and B(1, -3, 1, -3, 15, 1.0, 0.5) == 0   # n < 1
        assert B(1, 7, 3, 7, 15, 1.0, 0.5) == 0 and B(1, 7, 1, 6, 15, 1.0, 0.5) == 0 and B(1, 7, 7, 9, 15, 1.0, 0.5) == 0      # overlapping, not equal
        assert B(1, 7, 8, 9, 15, 1.0, 0.5) > 0 and B(8, 9, 1, 7, 15, 1.0, 0.5) > 0                                              # adjacent: disjoint
        assert B(1, 7, 1, 7, 0, 1.0, 0.5) == 0 and B(1, 7, 1, 7, 16, 1.0, 0.5) == 0                                             # plane mask
        for vmax in (0.0, -1.0, float("nan"), float("inf"), float(2 ** 20) + 1.0):
            assert B(1, 7, 1, 7, 15, vmax, 0.5) == 0
        assert B(1, 7, 1, 7, 15, float(2 ** 20), 0.5) == need
        assert B(1, 46341, 1, 46341, 8, 1.0, 0.5) == 0 and B(1, 46340, 1, 46340, 8, 1.0, 0.5) > 0                               # n_r n_c < 2^31
        assert B(-1, 7, -1, 7, 15, 1.0, 0.5) == 0
        for fn, tail in ((lib.matcha_pairmap_init, (None,)), (lib.matcha_pairmap_update, (p, p, None, 10, 3, None)),
                         (lib.matcha_pairmap_read, (1, p, p, None))):
            assert fn(None, need, *ok, *tail) == -22 and "null state" in err()
            assert fn(p, need - 1, *ok, *tail) == -22 and "too small" in err()
            assert fn(p, need, 1, 7, 3, 7, 15, 1.0, 0.5, *tail) == -22 and "disjoint" in err()
            assert fn(p, need, 1, 7, 1, 7, 15, 0.0, 0.5, *tail) == -22 and "vmax" in err()
        U = lib.matcha_pairmap_update
        for L in (1, 9, 0, -2):
            assert U(p, need, *ok, p, p, None, 10, L, None) == -22 and "width" in err()
        assert U(p, need, *ok, None, p, None, 10, 3, None) == -22 and "null x or value" in err()
        assert U(p, need, *ok, p, None, None, 10, 3, None) == -22 and "null x or value" in err()
        assert U(p, need, *ok, p, p, None, -1, 3, None) == -22 and "out of range" in err()
        R = lib.matcha_pairmap_read
        assert R(p, need, *ok, 1, None, p, None) == -22 and "null output" in err()
        assert R(p, need, *ok, 3, p, p, None) == -22 and "plane" in err()                                                      # two bits
        assert R(p, 512, 1, 7, 1, 7, 8, 1.0, 0.5, 1, p, p, None) == -22 and "plane" in err()                                    # not in the mask
        assert U(p, need, *ok, None, None, None, 0, 3, None) == 0                                                              # a no-op
    assert not log.counts
    with pytest.raises(_lib.MatchaHipError):
        SW.PairMap((1, 7), (1, 7), device="cpu")
    for kw in (dict(planes=0), dict(planes=["median"]), dict(planes=16)):
        with pytest.raises(ValueError):
            SW.PairMap((1, 7), (1, 7), device="cpu", **kw)


# ---- what the GPU test against the reference's logits rests on ---------------------------------------------------------------------
def test_golden_conditions_hold_on_the_reference_alone():
    g = gold("g11_kway_tiny.npz")
    ratios = []
    for i in range(3):
        for mode in ("table", "adj"):
            lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
            cut, gap = golden_cut(lg)
            tol = G11_TOL * np.abs(lg).max()
            assert gap >= 50 * tol, (mode, i, gap / tol)
            below, above = int((lg < cut).sum()), int((lg > cut).sum())
            assert below + above == len(lg) and len(lg) // 4 < below <= 3 * len(lg) // 4    # the cut is in the middle half
            ratios.append(int(gap / tol))
    assert sorted(ratios) == [62, 64, 72, 101, 119, 847]
    num = [int(v) for v in g["num"]]
    cr = np.asarray(synth.chrom_range(num))
    for i, (c, k, gap) in enumerate(g["cases"]):
        c, k, gap = int(c), int(k), int(gap)
        lo, n = int(cr[c][0]), int(cr[c][1] - cr[c][0])
        rows = g[f"rows_c{i}"]
        ref = pairmap_ref(rows, np.ones(len(rows), dtype=np.float32), (lo, n), (lo, n))
        cnt = np.zeros((n, n), dtype=np.int64)
        for row in itertools.combinations(range(lo, lo + n), k):
            if all(b - a >= gap for a, b in zip(row, row[1:])):
                for a, b in itertools.combinations(row, 2):
                    cnt[a - lo, b - lo] += 1
        assert np.array_equal(ref["count"], cnt + cnt.T)
        assert (int(cnt.max()), int((cnt > 0).sum())) == ((14, 120), (55, 105), (20, 85))[i]
        # the sweep's capacity rule: C(m, k - 2) bounds what one cell can receive
        m = n - (k - 1) * (gap - 1)
        import math
        assert cnt.max() <= math.comb(m, k - 2)
