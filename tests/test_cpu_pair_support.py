"""Per-pair support without a GPU (matcha_amd/sweep.py's SubsetPairSupport, csrc/sweep_support.hip's host side): the four entry
points and their refusals before any device call, the numpy twin (tests/pair_support_ref.py) against the per-locus twin in exact integers
and against a brute-force float64 sum on the g16 fixture's reference logits, and decomposition_sweep's argument refusals."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

from matcha_amd import _lib
from matcha_amd import sweep as SW
from tests import pair_support_ref as PS
from tests import subsets_ref as SR
from tests.helpers import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("matcha_subset_pair_bytes", "matcha_subset_pair_init", "matcha_subset_pair_update", "matcha_subset_pair_read")
PAIR_CASES = [i for i, case in enumerate(SR.G16_CASES) if case[1] >= 2]


def test_symbols_in_header_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "matcha_hip.h")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    for name in NEW:
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)
    assert PAIR_CASES == [0, 1, 2, 4]


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    odd = C.c_void_p(C.addressof(host) + 4)
    err = lambda: lib.matcha_last_error().decode()
    with _lib.launch_log() as log:
        need = lib.matcha_subset_pair_bytes(4, 9, 3, 1.0)
        assert need == 256 + 2 * 1280                                    # 8 * 4 * 36 = 1 152 bytes a plane, padded to a multiple of 256
        assert lib.matcha_subset_pair_bytes(5, 32, 8, 1.0) == 256 + 2 * 19968 and lib.matcha_subset_pair_bytes(1, 2, 2, 1048576.0) == 256 + 2 * 256
        for bad in ((0, 9, 3, 1.0), (4, 1, 3, 1.0), (4, 33, 3, 1.0), (4, 9, 1, 1.0), (4, 9, 9, 1.0), (4, 9, 3, 0.0), (4, 9, 3, float("nan")),
                    (4, 9, 3, float(1 << 21)), ((1 << 40) + 1, 9, 3, 1.0), (4, 9, 0, 1.0), (4, 9, 3, -1.0)):
            assert lib.matcha_subset_pair_bytes(*bad) == 0, bad
        assert lib.matcha_subset_pair_init(None, need, 4, 9, 3, 1.0, None) == -22 and "null state" in err()
        assert lib.matcha_subset_pair_init(odd, need, 4, 9, 3, 1.0, None) == -22 and "aligned" in err()
        assert lib.matcha_subset_pair_init(p, need - 1, 4, 9, 3, 1.0, None) == -22 and "too small" in err()
        assert lib.matcha_subset_pair_init(p, need, 4, 33, 3, 1.0, None) == -22 and "S" in err()
        assert lib.matcha_subset_pair_init(p, need, 4, 9, 1, 1.0, None) == -22 and "2 <= m" in err()                  # no pair in one position
        assert lib.matcha_subset_pair_update(None, need, 4, 9, 3, 1.0, p, None, 4, 0, None) == -22 and "null state" in err()
        assert lib.matcha_subset_pair_update(odd, need, 4, 9, 3, 1.0, p, None, 4, 0, None) == -22 and "aligned" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, None, None, 4, 0, None) == -22 and "null value" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, p, None, 4, 4 * 84 - 3, None) == -22 and "outside" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, p, None, 1, -1, None) == -22 and "outside" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, p, None, 1, (1 << 63) - 1, None) == -22 and "outside" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, p, None, -1, 0, None) == -22 and "n=" in err()
        assert lib.matcha_subset_pair_update(p, need - 8, 4, 9, 3, 1.0, p, None, 4, 0, None) == -22 and "too small" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, float("nan"), p, None, 4, 0, None) == -22 and "vmax" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 1, 1.0, p, None, 4, 0, None) == -22 and "2 <= m" in err()
        assert lib.matcha_subset_pair_read(p, need, 4, 9, 3, 1.0, None, None, None, None) == -22 and "null output" in err()
        assert lib.matcha_subset_pair_read(None, need, 4, 9, 3, 1.0, p, p, p, None) == -22 and "null state" in err()
        assert lib.matcha_subset_pair_read(odd, need, 4, 9, 3, 1.0, p, p, p, None) == -22 and "aligned" in err()
        assert lib.matcha_subset_pair_read(p, need - 1, 4, 9, 3, 1.0, p, p, p, None) == -22 and "too small" in err()
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, None, None, 0, 0, None) == 0                  # n = 0: nothing launched
        assert lib.matcha_subset_pair_update(p, need, 4, 9, 3, 1.0, p, p, 0, 4 * 84, None) == 0
    assert not log.counts
    with pytest.raises(_lib.MatchaHipError):
        SW.SubsetPairSupport(4, 9, 3, device="cpu")
    for S in (2, 3, 9, 32):
        i, j = SW.SubsetPairSupport.pair_index(S)
        assert len(i) == S * (S - 1) // 2 and bool((i < j).all())
        assert [PS.pair_cell(S, int(a), int(b)) for a, b in zip(i, j)] == list(range(len(i)))


def test_decomposition_sweep_refuses_pair_support_without_a_device():
    nine = [list(range(1, 10))] * 2
    with pytest.raises(ValueError, match="pair_support"):
        SW.decomposition_sweep(None, nine, 1, mode="drop", pair_support=True)
    with pytest.raises(ValueError, match="pair_support"):
        SW.decomposition_sweep(None, nine, 3, task_mode="regress", support=False, pair_support=True)
    with pytest.raises(ValueError):
        SW.decomposition_sweep(None, nine, 3, task_mode="regress", pair_support=True)


def awkward(rng, n):
    v = rng.random(n).astype(np.float32)
    at = rng.permutation(n)[:10]
    v[at] = [np.nan, -0.0, 1.0000001, np.inf, -np.inf, 1.0, 0.0, -1e-3, 1e-12, 0.5]
    skip = rng.random(n) < 0.2
    skip[at[:3]] = False
    skip[at[3]] = True
    return v, skip


@pytest.mark.parametrize("A,S,m", [(3, 5, 2), (4, 9, 3), (40, 8, 8), (2, 12, 5), (1, 32, 2)])
def test_twin_identities_in_exact_integers(A, S, m):
    """Summing the packed planes over all cells through position i gives (m - 1) x the per-locus planes (every chosen position pairs
    with the m - 1 others); the sum over all cells gives C(m, 2) x the accepted rows' totals; the cut is not part of the result."""
    cm = math.comb(S, m)
    n = A * cm
    rng = np.random.default_rng(S * 100 + m)
    v, skip = awkward(rng, n)
    total, cnt, counters = PS.pair_support(A, S, m, v, skip, 0)
    s_total, s_cnt, s_counters = SR.support(A, S, m, v, skip, 0)
    assert counters == s_counters and counters[1] >= 2
    full_t, full_c = PS.unpack(S, total), PS.unpack(S, cnt)
    assert np.array_equal(full_t.sum(axis=2), (m - 1) * s_total) and np.array_equal(full_c.sum(axis=2), (m - 1) * s_cnt)
    assert np.array_equal(full_t, full_t.transpose(0, 2, 1)) and not np.einsum("aii->ai", full_c).any()
    live = ~skip & (v >= 0) & (v <= 1)
    q = np.asarray([SR.quantum(x) if ok else 0 for x, ok in zip(v, live)], dtype=np.int64)
    pairs = m * (m - 1) // 2
    assert np.array_equal(cnt.sum(axis=1), pairs * live.reshape(A, cm).sum(axis=1))
    assert np.array_equal(total.sum(axis=1), pairs * q.reshape(A, cm).sum(axis=1))
    if m == 2:                                                           # a pair's rank is its cell
        assert np.array_equal(cnt.reshape(-1), live.astype(np.int64)) and np.array_equal(total.reshape(-1), q)
    state = None
    cuts = sorted({0, n // 3, n // 2 + 1, n})
    for lo, hi in reversed(list(zip(cuts, cuts[1:]))):
        state = PS.pair_support(A, S, m, v[lo:hi], skip[lo:hi], lo, state=state)
    assert np.array_equal(state[0], total) and np.array_equal(state[1], cnt) and state[2] == counters
    w = PS.pair_support(A, S, m, v, None, 0, vmax=2.0)
    assert w[2][0] + w[2][1] == n and w[2][0] > counters[0]


def g16_pair_reference(g, mode, i):
    """Per cluster of fixture case i: (s, float32 probabilities of all its candidates, valid mask, float64 [s, s] sums of the valid
    candidates' float32 probabilities per pair by brute force, int64 [s, s] counts, the same sums of the float64 probabilities)."""
    _, m, _, _, sizes = SR.G16_CASES[i]
    off, valid = g[f"offsets_c{i}"], g[f"valid_c{i}"]
    lg = g[f"logit_{mode}_c{i}"].astype(np.float64)
    out = []
    for a, s in enumerate(sizes):
        seg = slice(int(off[a]), int(off[a + 1]))
        p64 = 1.0 / (1.0 + np.exp(-lg[seg]))
        p = p64.astype(np.float32)
        want, cnt, want64 = np.zeros((s, s)), np.zeros((s, s), dtype=np.int64), np.zeros((s, s))
        for r, ch in enumerate(itertools.combinations(range(s), m)):
            if valid[seg][r]:
                for i0, j0 in itertools.combinations(ch, 2):
                    want[i0, j0] += np.float64(p[r])
                    want[j0, i0] += np.float64(p[r])
                    want64[i0, j0] += p64[r]
                    want64[j0, i0] += p64[r]
                    cnt[i0, j0] += 1
                    cnt[j0, i0] += 1
        out.append((s, p, valid[seg], want, cnt, want64))
    return out


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_twin_on_the_reference_logits(mode):
    g = gold("g16_subsets_tiny.npz")
    for i in PAIR_CASES:
        m = SR.G16_CASES[i][1]
        for s, p, valid, want, cnt, _ in g16_pair_reference(g, mode, i):
            total, count, counters = PS.pair_support(1, s, m, p, ~valid, 0)
            assert counters == [int(valid.sum()), 0]
            got_cnt, got = PS.unpack(s, count)[0], PS.unpack(s, total)[0].astype(np.float64) / SR.Q
            assert np.array_equal(got_cnt, cnt)
            assert (np.abs(got - want) <= cnt / SR.Q).all(), (mode, i, s)      # half a quantum per value, and float64's own rounding
