"""numpy restatement of one chromosome of denoise_contact.py (Code/denoise_contact.py:147-207) -- the checker of
matcha_amd/denoise.py and csrc/denoise.hip.  Every step is the reference's own numpy expression on float32 arrays; the quantile
transform is oracle.positives.quantile_uniform (scikit-learn's uniform QuantileTransformer fitted on every value).

Also the numpy twins of what the kernels implement: the pair offset of a row and its inverse, and the two summation orders of
np.mean (axis=-1: pairwise, in buffers of 8192; axis=0: one sequential chain per column)."""
import math

import numpy as np

from oracle.positives import quantile_uniform

EPS = 1e-15
BUF = 8192                   # numpy's reduction buffer (elements)
LEAF = 128                   # numpy's pairwise-sum block


# ---- pairs --------------------------------------------------------------------------------------------------------------
def pairs_ref(lo: int, hi: int, min_dis: int) -> np.ndarray:
    """generate_pair_wise (:67-74): (i, j), lo <= i, i + min_dis <= j < hi, row by row; int64 [n_pairs, 2]."""
    out = [[i, j] for i in range(lo, hi) for j in range(i + min_dis, hi)]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def pair_offset(r: int, n: int, min_dis: int) -> int:
    """First pair of row r (chromosome-relative); pair_offset(n, ...) is the pair count.  The kernels' closed form."""
    K = max(0, n - min_dis)
    rr = min(r, K)
    return rr * K - rr * (rr - 1) // 2


def pair_row(k: int, n: int, min_dis: int):
    """Inverse of pair_offset: (r, c) of pair k."""
    K = max(0, n - min_dis)
    # largest r with off(r) <= k: off(r) = r K - r (r - 1) / 2, solved in float64 and corrected by one step either way
    b = 2 * K + 1
    r = int((b - math.sqrt(max(0.0, b * b - 8.0 * k))) / 2)
    r = max(0, min(r, K - 1))
    while r > 0 and pair_offset(r, n, min_dis) > k:
        r -= 1
    while r + 1 < K and pair_offset(r + 1, n, min_dis) <= k:
        r += 1
    return r, r + min_dis + (k - pair_offset(r, n, min_dis))


# ---- numpy's summation orders -------------------------------------------------------------------------------------------------
def _pairwise(X: np.ndarray) -> np.ndarray:
    """numpy's pairwise sum of every row of X (float32), one buffer."""
    n = X.shape[1]
    if n < 8:
        s = np.full(X.shape[0], -0.0, dtype=np.float32)
        for k in range(n):
            s = s + X[:, k]
        return s
    if n <= LEAF:
        m = n - n % 8
        r = X[:, :8].copy()
        for i in range(8, m, 8):
            r = r + X[:, i:i + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for k in range(m, n):
            res = res + X[:, k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(X[:, :n2]) + _pairwise(X[:, n2:])


def row_sums_twin(X: np.ndarray) -> np.ndarray:
    """np.sum(X, axis=-1) of a C-contiguous float32 matrix: buffers of 8192 added in sequence, each summed pairwise."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    s = np.zeros(X.shape[0], dtype=np.float32)
    for c0 in range(0, X.shape[1], BUF):
        s = s + _pairwise(X[:, c0:c0 + BUF])
    return s


def col_sums_twin(X: np.ndarray) -> np.ndarray:
    """np.sum(X, axis=0): one float32 chain per column over the rows in order."""
    s = np.zeros(X.shape[1], dtype=np.float32)
    for r in range(X.shape[0]):
        s = s + X[r]
    return s


# ---- the post-processing ------------------------------------------------------------------------------------------------------
def assemble(rel_pairs: np.ndarray, values: np.ndarray, n: int) -> np.ndarray:
    """proba2matrix(pairs, None, values) (:31-62) with the pairs already chromosome-relative."""
    m = np.zeros((n, n), dtype="float32")
    m[rel_pairs[:, 0], rel_pairs[:, 1]] += values
    return m + m.T


def coverage(X: np.ndarray) -> np.ndarray:
    c1 = np.sqrt(np.mean(X, axis=-1, keepdims=True))
    c2 = np.sqrt(np.mean(X, axis=0, keepdims=True))
    X = X / (c1 + EPS)
    return X / (c2 + EPS)


def denoise_ref(proba: np.ndarray, origin_block: np.ndarray, n: int, min_dis: int, quantile_proba: bool = False):
    """One chromosome of n bins (relative ids 0 .. n-1): the same keys as matcha_amd.denoise.denoise_from_proba, as numpy."""
    proba = np.asarray(proba, dtype=np.float32).reshape(-1)
    origin_block = np.asarray(origin_block, dtype=np.float32)
    pw = pairs_ref(0, n, min_dis)
    if len(pw) == 0:
        return None
    weight = origin_block[pw[:, 0], pw[:, 1]]                      # origin[i - 1, j - 1] (:160)
    my_proba = coverage(assemble(pw, proba, n))                    # :162-166
    origin_raw = assemble(pw, weight, n)                           # :168
    gap1 = np.sum(origin_raw, axis=-1) == 0
    gap2 = np.sum(origin_raw, axis=0) == 0
    origin_part = coverage(origin_raw)                             # :171-174
    my = coverage(np.maximum(my_proba * origin_part, my_proba))    # :177-182
    my[gap1, :] = 0.0
    my[:, gap2] = 0.0
    my_proba[gap1, :] = 0.0
    my_proba[:, gap2] = 0.0
    my_q = quantile_uniform(my.reshape(-1)).reshape(n, n)          # :190-192 (fitted on every value)
    origin_q = quantile_uniform(origin_part.reshape(-1)).reshape(n, n)
    my_proba_q = quantile_uniform(my_proba.reshape(-1)).reshape(n, n) if quantile_proba else None
    return {"my": my, "origin_part": origin_part, "my_proba": my_proba, "gap1": gap1, "gap2": gap2, "my_q": my_q,
            "origin_q": origin_q, "my_proba_q": my_proba_q, "balanced": my_q[pw[:, 0], pw[:, 1]]}


# ---- fixture inputs (tests/golden/make_golden_denoise.py): regenerated from seeds, not stored ------------------------------------
FIXTURE_LAYOUTS = {"tiny": [16, 16, 16, 16], "mid": [100, 37, 64, 183]}
FIXTURE_RES = 1000000


def fixture_intra(num, seed: int) -> np.ndarray:
    """intra_adj float32 [N, N] of synth.make_adjacency with gaps: per chromosome a few bins whose row and column are zeroed
    (gap1 and gap2 of the reference), and in chromosome 0 one bin whose row alone is zeroed (a row that still has counts below
    the diagonal, so no gap)."""
    from matcha_amd import synth
    rng = np.random.default_rng(seed)
    intra, _ = synth.make_adjacency(rng, list(num))
    b = synth.bounds(list(num))
    for c in range(len(num)):
        lo, hi = b[c], b[c + 1]
        for k in rng.choice(np.arange(lo, hi), size=min(hi - lo, 1 + c % 2), replace=False):
            intra[k, :] = 0.0
            intra[:, k] = 0.0
    intra[b[1] - 2, :] = 0.0
    return intra


def fixture_node2bin(num, res: int = FIXTURE_RES):
    names = ["chr%d" % (c + 1) for c in range(len(num))]
    node2bin, node = {}, 1
    for c, n in enumerate(num):
        for k in range(n):
            node2bin[node] = "%s:%d" % (names[c], k * res)
            node += 1
    return node2bin, names
