"""The distance-matched expectation without a GPU (matcha_amd/expected.py, csrc/expected.hip's host side): the numpy
restatement (tests/expected_ref.py) against brute-force itertools, default_gap_edges, the tables against float64 formulas, save / load,
the overflow guard, the symbols, and the premise of the GPU test's set comparison on the
reference's own logits (g11)."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd import expected as EX
from tests import expected_ref as XR
from tests.helpers import gold
from tests.test_cpu_kway import brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                       # the device forward against the reference's CPU logits (tests/test_hip_kway.py)
EDGES = (2, 4, 8)
MIN_COUNT = 4
# (case, model) -> (K, gap of the sorted enrichment at K), computed from the fixture by the restatement and recorded in the issue
PREMISE = {(0, "table"): (23, 0.053), (0, "adj"): (13, 0.0083), (1, "table"): (37, 0.042), (1, "adj"): (15, 0.050),
           (2, "table"): (46, 0.26), (2, "adj"): (38, 0.0069)}


# ---- the restatement against brute force ---------------------------------------------------------------------------------------------
def brute_stratum(row, edges):
    """The definition, one candidate at a time, in Python integers."""
    G, s = len(edges) + 1, 0
    for a, b in zip(row, row[1:]):
        s = s * G + sum(1 for e in edges if e <= b - a)
    return s


def test_restatement_against_itertools_on_16_bin_regions():
    for lo in (1, 7):
        for k in (2, 3, 4, 5):
            for edges in ((), (2,), (2, 4, 8), (1, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 20, 99)):
                cands = [c for c in itertools.combinations(range(lo, lo + 16), k)]
                x = np.asarray(cands, dtype=np.int64)
                want = np.asarray([brute_stratum(c, edges) for c in cands], dtype=np.int32)
                got = XR.strata_ref(x, k, edges)
                assert np.array_equal(got, want), (lo, k, edges)
                assert got.min() >= 0 and got.max() < (len(edges) + 1) ** (k - 1)
                wide = np.concatenate([x, np.zeros((len(x), 2), dtype=np.int64)], axis=1)          # zero-padded rows: the same strata
                assert np.array_equal(XR.strata_ref(wide, k, edges), want)
                # a candidate read as one of another size, reversed, with a repeat or with a hole has no stratum
                assert (XR.strata_ref(wide, k + 1, edges) == -1).all()
                assert (XR.strata_ref(x[:, ::-1].copy(), k, edges) == -1).all()
                holed = wide.copy()
                holed[:, k + 1] = 5
                assert (XR.strata_ref(holed, k, edges) == -1).all()
                if k >= 3:
                    rep = x.copy()
                    rep[:, 1] = rep[:, 0]
                    assert (XR.strata_ref(rep, k, edges) == -1).all()
    # on and one below every edge
    for e in EDGES:
        assert XR.strata_ref(np.asarray([[5, 5 + e], [5, 5 + e - 1]]), 2, EDGES).tolist() == [EDGES.index(e) + 1, EDGES.index(e)]
    assert XR.strata_ref(np.asarray([[-3, 4, 9], [0, 4, 9], [1, 1 << 40, (1 << 40) + 1]]), 3, EDGES).tolist() == [-1, -1, 3 * 4 + 0]


def test_stats_restatement_against_python_integers():
    rng = np.random.default_rng(3)
    cands = np.asarray(brute(3, 16, 3, 1), dtype=np.int64)
    v = rng.random(len(cands)).astype(np.float32)
    v[:6] = np.asarray([0.0, -0.0, 1.0, np.nan, -1.0, 1.5], dtype=np.float32)
    skip = (rng.random(len(cands)) < 0.2).astype(np.int32)
    skip[:6] = 0
    for shift in (16, 32):
        ref = XR.stats_ref(cands, v, 3, EDGES, vmax=1.0, shift=shift, skip=skip)
        count, total, sq = [0] * 16, [0] * 16, [0] * 16
        n_rows = n_rej = 0
        for row, val, sk in zip(cands.tolist(), v.tolist(), skip.tolist()):
            if sk:
                continue
            if not 0.0 <= val <= 1.0:
                n_rej += 1
                continue
            s = brute_stratum(row, EDGES)
            n_rows += 1
            count[s] += 1
            total[s] += round(val * 2 ** shift)                          # exact: a float32 times a power of two; round half even = rint
            sq[s] += round(val * val * 2 ** shift)                      # exact too: 48 significant bits
        assert ref["count"].tolist() == count and ref["sum"].tolist() == total and ref["sumsq"].tolist() == sq
        assert (ref["n_rows"], ref["n_rejected"]) == (n_rows, n_rej) and n_rej == 3
        mean, var = XR.moments_ref(ref, shift)
        assert ((mean >= 0) & (mean <= 1)).all() and (var >= 0).all()


# ---- host code -----------------------------------------------------------------------------------------------------------------------
def test_default_gap_edges_properties():
    for k in range(2, 9):
        for n in (0, 1, 2, 3, 4, 5, 16, 17, 249, 1024, 1025, 2491):
            edges = EX.default_gap_edges(n, k)
            assert all(e < n for e in edges) and list(edges) == [2 ** (j + 1) for j in range(len(edges))]
            assert (len(edges) + 1) ** (k - 1) <= 1 << 20 and len(edges) <= 15
            full = [2 ** j for j in range(1, 40) if 2 ** j < n]
            if len(edges) < len(full):                                   # dropped only where it had to be: one more edge would not fit
                assert (len(edges) + 2) ** (k - 1) > 1 << 20 or len(edges) == 15
            st = EX.GapStrata(k, edges)
            assert st.n_strata == _lib.load().matcha_gap_strata_count(k, len(edges))
    assert EX.default_gap_edges(2491, 3) == (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
    assert EX.default_gap_edges(2491, 8) == (2, 4, 8, 16, 32, 64)
    with pytest.raises(ValueError):
        EX.default_gap_edges(100, 9)


def test_strata_object_and_decode():
    st = EX.GapStrata(3, EDGES)
    assert (st.G, st.n_strata, st.k, st.edges) == (4, 16, 3, EDGES)
    assert st.decode(0) == ((1, 1), (1, 1)) and st.decode(7) == ((2, 3), (8, None)) and st.decode(15) == ((8, None), (8, None))
    for s in range(16):                                                  # decode inverts the restatement: the lowest gaps of a stratum land in it
        lows = [lo for lo, _ in st.decode(s)]
        row = np.cumsum([5] + lows)[None, :]
        assert XR.strata_ref(row, 3, EDGES)[0] == s
        highs = [hi if hi is not None else 1000 for _, hi in st.decode(s)]
        assert XR.strata_ref(np.cumsum([5] + highs)[None, :], 3, EDGES)[0] == s
    assert EX.GapStrata(2, ()).n_strata == 1 and EX.GapStrata(2, ()).decode(0) == ((1, None),)
    assert EX.GapStrata(6, range(1, 16)).n_strata == 1 << 20
    for k, edges in ((1, EDGES), (9, EDGES), (3, (2, 2)), (3, (4, 2)), (3, (0, 2)), (3, (-1,)), (3, range(1, 17)), (7, range(1, 16)), (3, (1 << 63,))):
        with pytest.raises(ValueError):
            EX.GapStrata(k, edges)
    with pytest.raises(IndexError):
        st.decode(16)
    with pytest.raises(ValueError, match="cuda"):
        st.ids(torch.zeros(4, 3, dtype=torch.long))                      # no CPU fallback
    with pytest.raises(ValueError):
        EX.GapStats(st, device="cuda", shift=33)
    with pytest.raises(ValueError):
        EX.GapStats(st, device="cuda", vmax=0.0)
    with pytest.raises(ValueError, match="smaller shift"):
        EX.GapStats(st, device="cuda", vmax=float(1 << 20))
    with pytest.raises(ValueError):
        EX.GapStats(st, planes=["median"])
    with pytest.raises(_lib.MatchaHipError):
        EX.GapStats(st, device="cpu")


def make_expected(task_mode="class", with_var=True):
    count = np.asarray([0, 3, 4, 100, 7, 9, 50, 30] + [0] * 8, dtype=np.int64)
    mean = np.asarray([0.0, 0.2, 0.25, 0.9, 0.0, 1.0, 1e-6, 0.5] + [0.0] * 8)
    var = np.asarray([0.0, 0.01, 0.04, 0.0, 0.0, 0.0, 1e-12, 0.25] + [0.0] * 8)
    return EX.GapExpected(3, EDGES, 2, 3, task_mode, [(1, 17), (40, 60)], count, mean, var if with_var else None, 203, 5)


def test_table_modes_against_float64_formulas():
    ex = make_expected()
    nan = np.isnan
    off, sc = ex.table_host("logodds", 4)
    kept = [2, 3, 6, 7]                                                  # 0 empty, 1 undersampled, 4 E = 0, 5 E = 1
    assert np.flatnonzero(~nan(off)).tolist() == kept and off.dtype == sc.dtype == np.float32 and (sc == 1).all()
    for s in kept:
        E = ex.mean[s]
        assert off[s] == np.float32(math.log(E) - math.log1p(-E))
    assert abs(off[7]) < 1e-7 and off[6] == np.float32(math.log(1e-6) - math.log1p(-1e-6))
    off, sc = ex.table_host("ratio", 4)
    kept = [2, 3, 5, 6, 7]
    assert np.flatnonzero(~nan(off)).tolist() == kept and not off[kept].any()
    assert all(sc[s] == np.float32(1.0 / ex.mean[s]) for s in kept) and (sc[nan(off)] == 1).all()
    off, sc = ex.table_host("z", 4)
    kept = [2, 6, 7]                                                     # 3 and 5 have sd = 0
    assert np.flatnonzero(~nan(off)).tolist() == kept
    assert all(off[s] == np.float32(ex.mean[s]) and sc[s] == np.float32(1.0 / math.sqrt(ex.var[s])) for s in kept)
    assert np.flatnonzero(~nan(ex.table_host("ratio", 30)[0])).tolist() == [3, 6, 7]
    assert np.flatnonzero(~nan(ex.table_host("ratio", 0)[0])).tolist() == [1, 2, 3, 5, 6, 7]       # an empty stratum is always undersampled
    assert nan(ex.table_host("ratio", 101)[0]).all()
    for mode in EX.MODES:                                                # the restatement's table is the same table
        a, b = ex.table_host(mode, 4), XR.table_ref(ex.count, ex.mean, ex.var, mode, 4)
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        ex.table_host("median")
    with pytest.raises(ValueError, match="sumsq"):
        make_expected(with_var=False).table_host("z")
    with pytest.raises(ValueError, match="regress"):
        make_expected("regress").table_host("logodds")
    assert not nan(make_expected("regress").table_host("ratio", 4)[0][2])


def test_expected_save_load_round_trip(tmp_path):
    for with_var in (True, False):
        ex = make_expected(with_var=with_var)
        path = os.path.join(tmp_path, f"e{int(with_var)}.npz")
        ex.save(path)
        z = np.load(path, allow_pickle=False)                            # numbers and names only
        assert int(z["k"]) == 3 and z["edges"].tolist() == list(EDGES)
        back = EX.GapExpected.load(path)
        assert (back.k, back.edges, back.min_gap, back.width, back.task_mode, back.regions) == (3, EDGES, 2, 3, "class", ((1, 17), (40, 60)))
        assert np.array_equal(back.count, ex.count) and np.array_equal(back.mean, ex.mean) and (back.n_rows, back.n_rejected) == (203, 5)
        assert (back.var is None) == (not with_var) and (not with_var or np.array_equal(back.var, ex.var))
        for mode in ("logodds", "ratio"):
            a, b = ex.table_host(mode, 4), back.table_host(mode, 4)
            assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        EX.GapExpected(3, EDGES, 2, 3, "class", [], np.zeros(15, dtype=np.int64), np.zeros(15), None, 0, 0)


def test_result_raises_overflow_on_a_crafted_count():
    raw = {"count": np.asarray([5, 1 << 31, 0, 0], dtype=np.int64), "sum": np.zeros(4, dtype=np.int64), "sumsq": np.zeros(4, dtype=np.int64),
           "counters": np.asarray([(1 << 31) + 5, 0], dtype=np.int64)}
    with pytest.raises(OverflowError, match="smaller shift"):
        EX.stats_result(raw, 1.0, 32)                                    # 2^31 rows of up to 1.0 at 32 fractional bits: 2^63
    raw["count"][1] = (1 << 31) - 1
    out = EX.stats_result(raw, 1.0, 32)
    assert out["n_rows"] == (1 << 31) + 5 and out["mean"].tolist() == [0, 0, 0, 0] and out["var"].tolist() == [0, 0, 0, 0]
    assert EX.stats_result(dict(raw, count=np.asarray([1 << 40, 0, 0, 0])), 1.0, 16)["count"][0] == 1 << 40
    with pytest.raises(OverflowError):
        EX.stats_result(dict(raw, count=np.asarray([1 << 20, 0, 0, 0])), 1024.0, 24)      # vmax^2 2^24 = 2^44 per row
    # the arithmetic: sum / 2^shift / count, sumsq / 2^shift / count - mean^2
    raw = {"count": np.asarray([4, 0]), "sum": np.asarray([6 << 16, 0]), "sumsq": np.asarray([10 << 16, 0]), "counters": np.asarray([4, 1])}
    out = EX.stats_result(raw, 4.0, 16)
    assert out["mean"].tolist() == [1.5, 0.0] and out["var"].tolist() == [0.25, 0.0] and out["n_rejected"] == 1
    assert set(EX.stats_result({"count": raw["count"], "counters": raw["counters"]}, 1.0, 32)) == {"count", "n_rows", "n_rejected"}


def test_gap_symbols_in_header_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "matcha_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    want = {"matcha_gap_strata_count": 2, "matcha_gap_strata_ids": 8, "matcha_gap_stats_bytes": 3, "matcha_gap_stats_init": 6,
            "matcha_gap_stats_update": 14, "matcha_gap_stats_read": 10, "matcha_gap_enrich": 12}
    for name, n_args in want.items():
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name) and name in integ
        assert len(_lib.SIGNATURES[name][1]) == n_args
    for name, bit in (("COUNT", 1), ("SUM", 2), ("SUMSQ", 4), ("DIRECT", 8)):
        assert f"#define MATCHA_GAP_{name} {bit}" in hdr and getattr(_lib, f"GAP_{name}") == bit
    # the sizing arithmetic and the refusals, through ctypes (tests/host/expected_checks.hip repeats them under the sanitizers)
    assert lib.matcha_gap_strata_count(3, 3) == 16 and lib.matcha_gap_strata_count(6, 15) == 1 << 20 and lib.matcha_gap_strata_count(7, 15) == -1
    assert lib.matcha_gap_stats_bytes(3, 3, 7) == 1024 and lib.matcha_gap_stats_bytes(3, 3, 0) == 0 and lib.matcha_gap_stats_bytes(5, 15, 2) == 256 + (1 << 19)
    host = (C.c_int64 * 64)()
    p = C.cast(host, C.c_void_p)
    edges = (C.c_int64 * 3)(2, 8, 4)
    with _lib.launch_log() as log:
        assert lib.matcha_gap_stats_update(p, 1024, 3, C.cast(edges, C.c_void_p), 3, 7, 32, 1.0, p, 3, p, None, 4, None) == -22
        assert "strictly ascending" in lib.matcha_last_error().decode()
        assert lib.matcha_gap_stats_init(p, 1000, 3, 3, 7, None) == -22 and "matcha_gap_stats_bytes says 1024" in lib.matcha_last_error().decode()
        assert lib.matcha_gap_enrich(3, None, 0, p, 4, 2, p, p, p, None, p, None) == -22 and "L=2" in lib.matcha_last_error().decode()
    assert not log.counts


# ---- the premise of the GPU test's set comparison (tests/test_hip_expected.py) ------------------------------------------------------
def g11_reference(i, model):
    """(K, gap, tol, enrich, strata, count, offset) of fixture case i by the restatement on the reference's own logits."""
    g = gold("g11_kway_tiny.npz")
    _, k, _ = (int(v) for v in g["cases"][i])
    enrich, strata, offset, mean, count = XR.reference_enrichment(g[f"rows_c{i}"], g[f"logit_{model}_c{i}"], k, EDGES, MIN_COUNT)
    K, gap = XR.best_cut(enrich)
    return K, gap, XR.enrich_tolerance(mean, ~np.isnan(offset), TOL), enrich, strata, count, offset


@pytest.mark.parametrize("model", ["table", "adj"])
def test_premise_the_reference_top_k_is_separated_by_ten_tolerances(model):
    for i in range(3):
        K, gap, tol, enrich, strata, count, offset = g11_reference(i, model)
        want_K, want_gap = PREMISE[(i, model)]
        print(f"case {i} {model}: K={K} gap={gap:.4g} tol={tol:.4g}")
        assert K == want_K and abs(gap - want_gap) <= 0.05 * want_gap
        assert 10 <= K < 50 and gap >= 10 * tol                          # a device within tol of the reference selects the same K rows


def test_premise_strata_occupancy_of_the_fixture():
    g = gold("g11_kway_tiny.npz")
    occupied = []
    for i in range(3):
        _, k, _ = (int(v) for v in g["cases"][i])
        rows, logit = g[f"rows_c{i}"], g[f"logit_table_c{i}"]
        enrich, strata, offset, mean, count = XR.reference_enrichment(rows, logit, k, EDGES, MIN_COUNT)
        occupied.append((int((count > 0).sum()), len(count)))
        assert (strata >= 0).all() and count.sum() == len(rows)
        if i == 2:
            assert int((count >= MIN_COUNT).sum()) == 11 and int((~np.isnan(enrich)).sum()) == 52 and len(rows) == 56
        kept8 = int((~np.isnan(XR.reference_enrichment(rows, logit, k, EDGES, 8)[0])).sum())
        assert kept8 == (len(rows), 685, 0)[i] and len(rows) == (560, 715, 56)[i]           # c2 at min_count 8: the empty-result case
    assert occupied == [(15, 16), (17, 64), (15, 256)]
