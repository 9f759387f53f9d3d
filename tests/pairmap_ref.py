"""numpy restatement of the pair-map contract (include/matcha_hip.h): the oracle of csrc/pairmap.hip.

An accepted row contributes its value once per pair of positions ci < cj to the cell its two ids address; the sum is kept in fixed
point, int64 of rint(float64(v) * 2^32), accumulated with np.add.at (repeated cells DO accumulate, unlike the fancy-index ``+=`` of
the reference's proba2matrix); the maximum with np.maximum.at."""
import numpy as np

SCALE = float(1 << 32)


def pairmap_ref(x, value, rows, cols, vmax=1.0, threshold=0.5, skip=None):
    """x int64 [n, L], value float32 [n], rows = (lo_r, n_r), cols = (lo_c, n_c) equal or disjoint, skip int [n] or None.
    Returns dict(sum int64 raw, count, count_ge int64, max float32 with -inf where nothing landed, n_rows, n_rejected); a
    symmetric map comes mirrored with a zero diagonal."""
    x = np.asarray(x, dtype=np.int64)
    v = np.asarray(value, dtype=np.float32)
    (lo_r, n_r), (lo_c, n_c) = rows, cols
    symmetric = (lo_r, n_r) == (lo_c, n_c)
    assert symmetric or lo_r + n_r <= lo_c or lo_c + n_c <= lo_r
    skipped = np.zeros(len(v), dtype=bool) if skip is None else np.asarray(skip) != 0
    with np.errstate(invalid="ignore"):
        ok = (v >= np.float32(0)) & (v <= np.float32(vmax))               # False for NaN; -0.0 passes
    live = ~skipped & ok
    n_rows, n_rejected = int(live.sum()), int((~skipped & ~ok).sum())
    v = v + np.float32(0)                                                 # -0.0 counts as 0
    q = np.rint(v.astype(np.float64) * SCALE)
    s = np.zeros((n_r, n_c), dtype=np.int64)
    cnt = np.zeros((n_r, n_c), dtype=np.int64)
    ge = np.zeros((n_r, n_c), dtype=np.int64)
    mx = np.full((n_r, n_c), -np.inf, dtype=np.float32)
    L = x.shape[1]
    for ci in range(L - 1):
        for cj in range(ci + 1, L):
            a, b = x[:, ci], x[:, cj]
            pair = live & (a != 0) & (b != 0) & (a != b)
            if symmetric:
                hit = pair & (a >= lo_r) & (a < lo_r + n_r) & (b >= lo_r) & (b < lo_r + n_r)
                r, c = np.minimum(a, b) - lo_r, np.maximum(a, b) - lo_r
            else:
                fwd = (a >= lo_r) & (a < lo_r + n_r) & (b >= lo_c) & (b < lo_c + n_c)
                rev = (b >= lo_r) & (b < lo_r + n_r) & (a >= lo_c) & (a < lo_c + n_c)
                hit = pair & (fwd | rev)
                r, c = np.where(fwd, a, b) - lo_r, np.where(fwd, b, a) - lo_c
            r, c, vv, qq = r[hit], c[hit], v[hit], q[hit].astype(np.int64)
            np.add.at(s, (r, c), qq)
            np.add.at(cnt, (r, c), 1)
            np.add.at(ge, (r, c), (vv >= np.float32(threshold)).astype(np.int64))
            np.maximum.at(mx, (r, c), vv)
    if symmetric:
        up = np.triu(np.ones((n_r, n_r), dtype=bool), 1)
        assert not s[~up].any() and not cnt[~up].any()
        s, cnt, ge = s + s.T, cnt + cnt.T, ge + ge.T
        mx = np.where(up, mx, mx.T)
        np.fill_diagonal(mx, 0.0)
    return dict(sum=s, count=cnt, count_ge=ge, max=mx, n_rows=n_rows, n_rejected=n_rejected)


def golden_cut(logits):
    """The cut of a golden logit vector for the exact count_ge test: the midpoint of the largest gap between consecutive sorted
    logits among positions n//4 .. 3n//4 of the sorted list.  Returns (cut, gap)."""
    s = np.sort(np.asarray(logits, dtype=np.float64))
    n = len(s)
    a, b = n // 4, 3 * n // 4
    gaps = s[a + 1:b + 1] - s[a:b]
    j = a + int(np.argmax(gaps))
    return 0.5 * (s[j] + s[j + 1]), float(s[j + 1] - s[j])


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))
