"""The multi-region sweep without a GPU (matcha_amd/sweep.py, csrc/sweep_rows.hip's host side): the two entry points and their
refusals before any device call, region_count / region_unrank against itertools, the g18 fixture's consistency, the wrappers' and the
CLI parser's checks.  (The host side alone under ASan + UBSan: tests/test_cpu_host_checks.py.)"""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR, synth
from matcha_amd import sweep as SW
from tests import regions_ref as RR
from tests.helpers import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (parts, min_gap): the fixture's cases in node ids of the tiny layout, then the shapes the kernel treats differently
TINY = np.asarray(synth.chrom_range(synth.LAYOUTS["tiny"]))
GRID = [(RR.case_parts(case, TINY), gap) for case, gap in RR.CASES] + [
    ([(5, 21, 3)], 2),                                                   # P = 1: kway_rows' rows
    ([(5, 21, 2)], 1),
    ([(1 + 4 * p, 4 + 4 * p, 1) for p in range(8)], 1),                  # P = 8, every part a single bin of 3: 3^8 = 6 561
    ([(1 + 4 * p, 4 + 4 * p, 1) for p in range(8)], 3),                  # ... of which the gap rule leaves few
    ([(3, 15, 8)], 1),                                                   # one part of 8: C(12, 8) = 495
    ([(3, 15, 8)], 2),                                                   # C(5, 8) = 0
    ([(1, 7, 3), (40, 56, 2)], 4),                                       # C(0, 3) = 0 in one part: T = 0
    ([(1, 9, 2), (9, 15, 1), (15, 23, 2)], 3),                           # three regions that touch: invalid exactly at the boundaries
    ([(1, 9, 1), (10, 14, 2), (14, 20, 1)], 2),
    ([(2, 9, 3), (30, 33, 1), (50, 58, 4)], 1),                          # k = 8 over three parts
]


def part_arrays(parts):
    P = len(parts)
    lo = (C.c_int64 * P)(*[a for a, _, _ in parts])
    n = (C.c_int32 * P)(*[b - a for a, b, _ in parts])
    m = (C.c_int32 * P)(*[c for _, _, c in parts])
    return P, lo, n, m                                                   # the arrays stay alive with the tuple


def lib_count(parts, gap):
    P, lo, n, m = part_arrays(parts)
    return _lib.load().matcha_kway_region_count(P, C.cast(lo, C.c_void_p), C.cast(n, C.c_void_p), C.cast(m, C.c_void_p), gap)


def test_region_symbols_in_header_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "matcha_hip.h")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("matcha_kway_region_count", "matcha_kway_region_rows"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["matcha_kway_region_count"][1]) == 5 and len(_lib.SIGNATURES["matcha_kway_region_rows"][1]) == 12
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "matcha_kway_region_rows" in integ and "matcha_kway_region_count" in integ


def test_region_rows_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()

    def rows(parts, gap, rank0, ranks, count, L, x=p, flag=p, P=None, drop=None):
        n_parts, lo, n, m = part_arrays(parts)
        arrays = [C.cast(a, C.c_void_p) for a in (lo, n, m)]
        if drop is not None:
            arrays[drop] = None
        return lib.matcha_kway_region_rows(n_parts if P is None else P, *arrays, gap, rank0, ranks, count, L, x, flag, None)

    two = [(1, 17, 1), (33, 49, 2)]                                      # 1 920 candidates
    big = [(0, 1 << 21, 1), (1 << 31, (1 << 31) + (1 << 21), 1), (1 << 32, (1 << 32) + (1 << 21), 1)]      # 2^63 exactly
    with _lib.launch_log() as log:
        assert rows(two, 1, 0, None, 4, 3, P=0) == -22 and "P=0" in err()
        assert rows(two, 1, 0, None, 4, 3, P=9) == -22 and "P=9" in err()
        for drop in range(3):
            assert rows(two, 1, 0, None, 4, 3, drop=drop) == -22 and "null part arrays" in err()
        assert rows(two, 0, 0, None, 4, 3) == -22 and "min_gap=0" in err()
        assert rows([(1, 17, 0), (33, 49, 2)], 1, 0, None, 4, 3) == -22 and "part 0" in err() and "m=0" in err()
        assert rows([(1, 17, 1), (33, 33, 2)], 1, 0, None, 4, 3) == -22 and "part 1" in err() and "n=0" in err()
        assert rows([(1, 17, 1)], 1, 0, None, 4, 3) == -22 and "k=1" in err()
        assert rows([(1, 17, 4), (33, 49, 5)], 1, 0, None, 4, 8) == -22 and "k=9" in err()
        assert rows([(1, 17, 1), (16, 49, 2)], 1, 0, None, 4, 3) == -22 and "ascending and disjoint" in err()
        assert rows([(33, 49, 1), (1, 17, 2)], 1, 0, None, 4, 3) == -22 and "ascending and disjoint" in err()
        assert rows([(-1, 17, 1), (33, 49, 2)], 1, 0, None, 4, 3) == -22 and "lo of part 0" in err()
        assert rows([(1, 17, 1), ((1 << 62) + 1, (1 << 62) + 17, 2)], 1, 0, None, 4, 3) == -22 and "lo of part 1" in err()
        assert rows(two, 1, 0, None, 4, 2) == -22 and "L=2" in err()
        assert rows(two, 1, 0, None, 4, 9) == -22 and "L=9" in err()
        assert rows(big, 1, 0, None, 4, 3) == -22 and "63 bits" in err()
        assert rows([(0, (1 << 31) - 1, 8)], 1, 0, None, 4, 8) == -22 and "63 bits" in err()
        assert rows(two, 1, 1918, None, 4, 3) == -22 and "outside" in err()
        assert rows(two, 1, -1, None, 1, 3) == -22 and "outside" in err()
        assert rows(two, 1, 1921, None, 0, 3) == -22 and "outside" in err()
        assert rows([(3, 15, 8)], 2, 0, None, 1, 8) == -22 and "outside" in err()            # T = 0: no rank exists
        assert rows(two, 1, 0, None, -1, 3) == -22 and "count" in err()
        assert rows(two, 1, 0, p, (1 << 40) + 1, 3) == -22 and "count" in err()
        assert rows(two, 1, 0, None, 4, 3, x=None) == -22 and "null output" in err()
        assert rows(two, 1, 0, None, 4, 3, flag=None) == -22 and "null output" in err()
        # the no-op forms
        assert rows(two, 1, 0, None, 0, 3, x=None, flag=None) == 0 and rows(two, 1, 1920, None, 0, 8, x=None, flag=None) == 0
        assert rows(two, 1, 0, p, 0, 3, x=None, flag=None) == 0                              # an empty list of ranks
        assert rows([(3, 15, 8)], 2, 0, None, 0, 8, x=None, flag=None) == 0                  # T = 0
        just_below = big[:2] + [(1 << 32, (1 << 32) + (1 << 21) - 1, 1)]
        assert rows(just_below, 1, (1 << 42) * ((1 << 21) - 1), None, 0, 3, x=None, flag=None) == 0
    assert not log.counts


def test_region_count_and_unrank_against_itertools():
    for parts, gap in GRID:
        ref, valid = RR.candidates(parts, gap)
        T = SW.region_count(parts, gap)
        assert T == len(ref) == lib_count(parts, gap), (parts, gap)
        got = [SW.region_unrank(r, parts, gap) for r in range(T)]
        assert [row for row, _ in got] == [tuple(r) for r in ref.tolist()], (parts, gap)
        assert [ok for _, ok in got] == valid.tolist(), (parts, gap)
        rows = [row for row, _ in got]
        assert all(a < b for a, b in zip(rows, rows[1:]))                # rank order is the lexicographic order of the rows
        assert all(all(x < y for x, y in zip(r, r[1:])) for r in rows)   # every row ascends as it stands
        # the invalid ranks are exactly the violations at a part boundary; inside a part the rule holds by construction
        ends = np.cumsum([m for _, _, m in parts])[:-1]
        if len(ref):
            d = np.diff(ref, axis=1)
            inner = np.delete(d, ends - 1, axis=1)
            assert (inner >= gap).all() and np.array_equal(valid, (d[:, ends - 1] >= gap).all(axis=1))
        for bad in (-1, T):
            with pytest.raises(IndexError):
                SW.region_unrank(bad, parts, gap)
    touching = [g for g in GRID if any(a[1] == b[0] for a, b in zip(g[0], g[0][1:]))]
    assert all(0 < (~RR.candidates(*g)[1]).sum() < len(RR.candidates(*g)[1]) for g in touching) and len(touching) >= 3
    assert sum(SW.region_count(*g) == 0 for g in GRID) == 2


def test_region_one_part_is_kway():
    for lo, n, k, gap in ((5, 16, 3, 2), (5, 16, 2, 1), (3, 12, 8, 1), (9, 30, 4, 3)):
        parts = [(lo, lo + n, k)]
        T = SW.region_count(parts, gap)
        assert T == SW.kway_count(n, k, gap) > 0
        for r in list(range(0, T, max(1, T // 97))) + [T - 1]:
            assert SW.region_unrank(r, parts, gap) == (SW.kway_unrank(r, lo, n, k, gap), True)


def test_region_large_spaces_and_the_63_bit_refusal():
    eight = [(1 + 200 * p, 201 + 200 * p, 1) for p in range(8)]
    T = SW.region_count(eight, 1)
    assert T == 200 ** 8 == lib_count(eight, 1) and T > 1 << 61
    for r in (0, 1, 199, 200, T // 3, T - 201, T - 1):
        digits = [(r // 200 ** (7 - p)) % 200 for p in range(8)]
        assert SW.region_unrank(r, eight, 1) == (tuple(1 + 200 * p + d for p, d in enumerate(digits)), True)
    assert SW.region_unrank(199, eight, 2) == (tuple([1, 201, 401, 601, 801, 1001, 1201, 1600]), True)
    assert SW.region_unrank(200 * 199, eight, 2)[1] is False             # ... 1400, 1401: one apart
    # mixed: a part of 4 with a 2^40-sized count beside single bins
    mixed = [(1, 2492, 4), (3000, 3100, 1), (4000, 4007, 2)]
    T = SW.region_count(mixed, 2)
    c0, c2 = math.comb(2491 - 3, 4), math.comb(6, 2)
    assert T == c0 * 100 * c2 == lib_count(mixed, 2) and c0 > 1 << 40
    r = (c0 - 5) * 100 * c2 + 37 * c2 + 4
    row, ok = SW.region_unrank(r, mixed, 2)
    assert row[:4] == SW.kway_unrank(c0 - 5, 1, 2491, 4, 2) and row[4] == 3037 and row[5:] == SW.kway_unrank(4, 4000, 7, 2, 2) and ok
    # T >= 2^63 is refused, not truncated, by the library and by the wrapper
    big = [(0, 1 << 21, 1), (1 << 31, (1 << 31) + (1 << 21), 1), (1 << 32, (1 << 32) + (1 << 21), 1)]
    assert lib_count(big, 1) == -1
    with pytest.raises(ValueError, match="63 bits"):
        SW.region_count(big, 1)
    with pytest.raises(ValueError, match="63 bits"):
        SW.region_unrank(0, big, 1)
    below = big[:2] + [(1 << 32, (1 << 32) + (1 << 21) - 1, 1)]
    assert SW.region_count(below, 1) == lib_count(below, 1) == (1 << 42) * ((1 << 21) - 1)
    assert lib_count([(0, (1 << 31) - 1, 8)], 1) == -1
    assert lib_count([(0, (1 << 31) - 1, 6), (1 << 31, (1 << 31) + 3, 2)], 5) == -1          # an overflowing part beside an empty one


def test_region_wrappers_refuse_before_any_launch():
    two = [(1, 17, 1), (33, 49, 2)]
    bad_parts = ([], [(1, 17, 1)] * 9, [(1, 17, 0), (33, 49, 2)], [(1, 1, 1), (33, 49, 2)], [(1, 17, 1)], [(1, 17, 4), (33, 49, 5)],
                 [(1, 17, 1), (16, 49, 2)], [(33, 49, 1), (1, 17, 2)], [(-1, 17, 1), (33, 49, 2)], [(1, 17)], [(0, 1 << 31, 1), (1 << 40, (1 << 40) + 5, 1)])
    with _lib.launch_log() as log:
        for parts in bad_parts:
            for fn in (SW.region_count, lambda p, g: SW.region_unrank(0, p, g), SW.region_rows, lambda p, g: SW.region_sweep(None, p, g, top=5),
                       lambda p, g: SW.region_map(None, p, g, 0, 1)):
                with pytest.raises(ValueError):
                    fn(parts, 1)
        for fn in (SW.region_count, SW.region_rows):
            with pytest.raises(ValueError):
                fn(two, 0)
            assert lib_count(two, 0) == -1
        for kw in (dict(width=2), dict(width=9)):
            with pytest.raises(ValueError):
                SW.region_rows(two, 1, **kw)
        for kw in (dict(rank0=1918, count=4), dict(rank0=-1, count=1), dict(count=-1), dict(rank0=1921, count=0)):
            with pytest.raises(IndexError):
                SW.region_rows(two, 1, **kw)
        for kw in (dict(out=torch.zeros(10, dtype=torch.long)), dict(out=torch.zeros(40, dtype=torch.int32)),
                   dict(out=torch.zeros(40, dtype=torch.long), flag_out=torch.zeros(3, dtype=torch.int32)),
                   dict(out=torch.zeros(40, dtype=torch.long), flag_out=torch.zeros(8, dtype=torch.long))):
            with pytest.raises(ValueError):
                SW.region_rows(two, 1, count=4, **kw)
        with pytest.raises(_lib.MatchaHipError):
            SW.region_rows(two, 1, count=4, device="cpu")               # every argument is fine: no CPU fallback
        # the drivers check their arguments before they touch the model
        for kw in (dict(top=0), dict(top=5, chunk_rows=0), dict(top=5, width=2), dict(top=5, width=9), dict(top=5, task_mode="other")):
            with pytest.raises(ValueError):
                SW.region_sweep(None, two, 1, **kw)
        with pytest.raises(ValueError, match="per_leading"):
            SW.region_sweep(None, [(5, 21, 3)], 1, top=5, per_leading=True)
        for args, kw in (((0, 2), {}), ((-1, 1), {}), ((0, 0), {}), ((0, 1), dict(chunk_rows=0)), ((0, 1), dict(width=9)), ((0, 1), dict(task_mode="other")),
                         ((0, 1), dict(task_mode="regress")), ((0, 1), dict(task_mode="regress", value_max=float(1 << 21))), ((0, 1), dict(planes="other"))):
            with pytest.raises(ValueError):
                SW.region_map(None, two, 1, *args, **kw)
        # the capacity bound: rectangular, prod of the other parts' counts C(n_r - 1, m_r - 1) C(n_c - 1, m_c - 1); symmetric, C(n_r - 2, m_r - 2)
        wide = [(1, 3001, 1), (4000, 7000, 1), (8000, 11000, 2)]
        assert SW.region_map_bound(wide, 1, 0, 1) == math.comb(3000, 2) and SW.region_map_bound(wide, 1, 0, 2) == 3000 * 2999
        assert SW.region_map_bound(wide, 1, 2, 2) == 3000 * 3000 and SW.region_map_bound(two, 1, 0, 1) == 15 and SW.region_map_bound(two, 1, 1, 1) == 16
        huge = [(1, 60001, 1), (70000, 140000, 2), (150000, 210000, 1)]
        assert SW.region_map_bound(huge, 1, 0, 2) == math.comb(70000, 2) >= 1 << 31 and SW.region_count(huge, 1) < 1 << 63
        with pytest.raises(ValueError, match="capacity"):
            SW.region_map(None, huge, 1, 0, 2)
        assert SW.region_map_bound(huge, 1, 1, 1) == 60000 * 60000      # the other two parts' counts, C(n - 2, 0) = 1
    assert not log.counts


def test_region_map_bound_is_never_too_small():
    """Brute force: the largest number of VALID candidates through one cell never exceeds the bound."""
    for parts, gap in GRID:
        rows, valid = RR.candidates(parts, gap)
        if not len(rows):
            continue
        cols = np.cumsum([0] + [m for _, _, m in parts])
        for r, c in itertools.product(range(len(parts)), repeat=2):
            if r == c and parts[r][2] < 2:
                continue
            cells = {}
            for row in rows[valid].tolist():
                a_ids, b_ids = row[cols[r]:cols[r + 1]], row[cols[c]:cols[c + 1]]
                pairs = itertools.combinations(a_ids, 2) if r == c else itertools.product(a_ids, b_ids)
                for pair in pairs:
                    cells[pair] = cells.get(pair, 0) + 1
            assert max(cells.values(), default=0) <= SW.region_map_bound(parts, gap, r, c), (parts, gap, r, c)


def test_region_fixture_is_self_consistent():
    g = gold("g18_regions_tiny.npz")
    assert [int(v) for v in g["num"]] == [16, 16, 16, 16] and int(g["n_cases"]) == len(RR.CASES) == 4
    want = [(1920, 3), (1344, 4), (168, 4), (2646, 5)]
    for i, (case, gap) in enumerate(RR.CASES):
        parts = RR.case_parts(case, TINY)
        assert np.array_equal(g[f"parts_c{i}"], np.asarray(parts)) and int(g[f"gap_c{i}"]) == gap
        rows, valid = RR.candidates(parts, gap)
        assert (len(rows), rows.shape[1]) == want[i] and SW.region_count(parts, gap) == len(rows)
        assert np.array_equal(g[f"valid_c{i}"].astype(bool), valid) and int(g[f"ninvalid_c{i}"]) == int((~valid).sum())
        assert (int(g[f"ninvalid_c{i}"]) > 0) == (i == 2)
        for mode in ("table", "adj"):
            ref = g[f"logit_{mode}_c{i}"]
            assert ref.dtype == np.float32 and ref.shape == (len(rows),) and len(np.unique(ref)) == len(ref)
            K = int(g[f"ksel_{mode}_c{i}"])
            s = np.sort(ref[valid].astype(np.float64))[::-1]
            assert 10 <= K < 50 and (s[K - 1] - s[K]) / np.abs(s).max() >= 100 * 1e-4


def test_region_cli_part_parser():
    names = ["chr1", "chr2", "chr3", "chr4"]
    assert PR.parse_parts(["0:1", "chr3:2:0-8", "3:1"], TINY, names) == [(1, 17, 1), (33, 41, 2), (49, 65, 1)]
    assert PR.parse_parts(["1:2:0-6", "1:2:6-16"], TINY, names) == [(17, 23, 2), (23, 33, 2)]
    for specs, word in ((["0"], "--part 0:"), (["0:1", "x:1"], "--part x:1"), (["7:1"], "--part 7:1"), (["0:a"], "--part 0:a"), (["0:0"], "--part 0:0"),
                        (["0:1:3"], "--part 0:1:3"), (["0:1:5-5"], "--part 0:1:5-5"), (["0:1:0-17"], "--part 0:1:0-17"), (["0:1:a-b"], "--part 0:1:a-b"),
                        (["2:1", "0:1"], "--part 0:1"), (["1:2:0-8", "1:1:7-12"], "--part 1:1:7-12"), (["0:1", "2:1", "2:2"], "--part 2:2"),
                        ([], "--part")):
        with pytest.raises(ValueError) as e:
            PR.parse_parts(specs, TINY, names)
        assert word in str(e.value), (specs, str(e.value))
