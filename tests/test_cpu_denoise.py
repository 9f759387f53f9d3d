"""The denoised contact maps on the CPU: tests/denoise_ref.py against the REAL denoise_contact.py (gd_* fixtures,
tests/golden/make_golden_denoise.py), and the numpy twins of what csrc/denoise.hip implements -- numpy's two summation orders of
np.mean and the closed-form pair offset -- against numpy and generate_pair_wise themselves."""
import numpy as np
import pytest

from matcha_amd import synth
from matcha_amd.denoise import cooler_tables, pair_count
from tests import denoise_ref as R
from tests.helpers import gold

CASES = ["tiny_table_md2", "tiny_adj_md0", "tiny_table_regress", "mid_table_md2"]
MATS = ["my", "origin_part", "my_proba", "gap1", "gap2", "my_q", "origin_q", "my_proba_q", "balanced"]


def fixture(case):
    """{key: array} of one gd_* case, its per-chromosome files merged."""
    g = dict(gold(f"gd_{case}.npz"))
    for c in range(len(g["num"])):
        try:
            g.update(dict(gold(f"gd_{case}_c{c}.npz")))
        except FileNotFoundError:
            pass
    return g


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("case", CASES)
def test_reference_restatement_matches_fixture_bitwise(case):
    g = fixture(case)
    num, min_dis = [int(v) for v in g["num"]], int(g["min_dis"])
    intra = R.fixture_intra(num, int(g["seed"]))
    b = synth.bounds(num)
    n_gaps = 0
    for c, n in enumerate(num):
        got = R.denoise_ref(g[f"proba_c{c}"], intra[b[c]:b[c + 1], b[c]:b[c + 1]], n, min_dis, quantile_proba=True)
        for k in MATS:
            key = f"{k}_c{c}"
            if key in g:
                assert same(got[k], g[key]), f"{case} chromosome {c}: {k}"
        assert len(g[f"proba_c{c}"]) == pair_count(n, min_dis)
        n_gaps += int(g[f"gap1_c{c}"].sum())
    assert n_gaps >= len(num)                           # every chromosome has a zeroed bin


@pytest.mark.parametrize("case", CASES)
def test_cooler_tables_match_fixture(case):
    g = fixture(case)
    num, res = [int(v) for v in g["num"]], int(g["res"])
    node2bin, names = R.fixture_node2bin(num, res)
    chrom, start, end, cn = cooler_tables(node2bin, names, res)
    p = f"ds/resolutions/{res}/"
    assert np.array_equal(chrom, g[p + "bins/chrom"]) and np.array_equal(start, g[p + "bins/start"])
    assert np.array_equal(end, g[p + "bins/end"])
    assert [s.decode() if isinstance(s, bytes) else str(s) for s in g[p + "chroms/name"]] == cn
    # pixels: bin ids i - 1, j - 1 over the chromosomes, balanced the concatenation of the per-chromosome pixels
    cr = synth.chrom_range(num)
    ids = np.concatenate([R.pairs_ref(int(lo), int(hi), int(g["min_dis"])) for lo, hi in cr]) - 1
    assert np.array_equal(ids[:, 0], g[p + "pixels/bin1_id"]) and np.array_equal(ids[:, 1], g[p + "pixels/bin2_id"])
    bal = np.concatenate([g[f"balanced_c{c}"] for c in range(len(num))])
    assert same(bal, g[p + "pixels/balanced"])


SUM_SIZES = list(range(1, 301)) + [511, 512, 513, 1000, 2491]


def test_summation_twins_match_numpy():
    """np.mean(axis=-1) is numpy's pairwise sum (buffers of 8192) / n; np.mean(axis=0) one sequential chain per column / n.  If a future
    numpy changes its order, this test names the cause of a bitwise failure elsewhere."""
    rng = np.random.default_rng(5)
    for n in SUM_SIZES:
        rows = min(n, 24)
        X = (rng.random((rows, n), dtype=np.float32) * rng.choice(np.array([1e-3, 1.0, 1e3], np.float32), size=(rows, n))).astype(np.float32)
        X[:, rng.random(n) < 0.1] = 0.0
        assert same(R.row_sums_twin(X) / np.float32(n), np.mean(X, axis=-1)), n
        Y = X.T.copy() if rows == n else rng.random((n, rows), dtype=np.float32)
        assert same(R.col_sums_twin(Y) / np.float32(n), np.mean(Y, axis=0)), n


@pytest.mark.parametrize("n", [8192, 8193, 9000, 16385])
def test_row_sums_twin_beyond_one_buffer(n):
    """Above 8192 columns numpy reduces a row in buffers of 8192 added in sequence (the kernels' outer loop)."""
    rng = np.random.default_rng(n)
    X = (rng.random((64, n), dtype=np.float32) * rng.choice(np.array([1e-3, 1.0, 1e3], np.float32), size=(64, n))).astype(np.float32)
    assert same(R.row_sums_twin(X), np.sum(X, axis=-1))
    if n > 8192:                                                       # one pairwise tree over the whole row is NOT numpy's order
        assert not same(R._pairwise(X), np.sum(X, axis=-1))


def test_pair_offset_and_inverse_match_generate_pair_wise():
    for n in range(1, 71):
        for md in sorted({0, 1, 2, 5, n - 1, n, n + 3}):
            if md < 0:
                continue
            pw = R.pairs_ref(0, n, md)
            assert len(pw) == pair_count(n, md) == R.pair_offset(n, n, md)
            for r in range(n):
                cnt = max(0, n - r - md)
                first = R.pair_offset(r, n, md)
                if cnt:
                    assert pw[first, 0] == r and pw[first + cnt - 1, 0] == r and pw[first, 1] == r + md
            for k in range(len(pw)):
                assert R.pair_row(k, n, md) == (pw[k, 0], pw[k, 1])


def test_empty_chromosome_has_no_pixels():
    assert R.denoise_ref(np.zeros(0, np.float32), np.zeros((3, 3), np.float32), 3, 3) is None
    assert pair_count(3, 3) == 0 and pair_count(3, 7) == 0 and pair_count(3, 2) == 1
