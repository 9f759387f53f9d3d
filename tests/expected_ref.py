"""numpy restatement of the distance-matched expectation (include/matcha_hip.h): the oracle of csrc/expected.hip and
of matcha_amd/expected.py.  Strata from the definition, the planes in integer arithmetic with the kernel's rint, the tables in float64
and the enrichment in float32 -- nothing here calls the code under test."""
import numpy as np


def strata_ref(x, k, edges):
    """int32 [n]: the stratum of every row of x int64 [n, L]; -1 for a row whose leading non-zero run is not exactly k ids, is not
    strictly ascending (or starts below 1), or is followed by a non-zero id after a zero."""
    x = np.asarray(x, dtype=np.int64)
    n, L = x.shape
    edges = np.asarray(list(edges), dtype=np.int64)
    G = len(edges) + 1
    out = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        row = [int(v) for v in x[i]]
        run = 0
        while run < L and row[run] != 0:
            run += 1
        if run != k or any(v != 0 for v in row[run:]) or row[0] < 1:
            continue
        if any(b <= a for a, b in zip(row[:k], row[1:k])):
            continue
        s = 0
        for a, b in zip(row[:k], row[1:k]):
            s = s * G + int(np.searchsorted(edges, b - a, side="right"))
        out[i] = s
    return out


def stats_ref(x, value, k, edges, vmax=1.0, shift=32, skip=None):
    """dict(count, sum, sumsq int64 [G^(k-1)], n_rows, n_rejected): an accepted row (not skipped, stratum >= 0, 0 <= v <= vmax with
    -0.0 counting as 0) adds 1, rint(float64(v) 2^shift) and rint(float64(v)^2 2^shift) to its stratum."""
    v = np.asarray(value, dtype=np.float32)
    s = strata_ref(x, k, edges)
    n_strata = (len(list(edges)) + 1) ** (k - 1)
    skipped = np.zeros(len(v), dtype=bool) if skip is None else np.asarray(skip) != 0
    with np.errstate(invalid="ignore"):
        ok = (s >= 0) & (v >= np.float32(0)) & (v <= np.float32(vmax))   # False for NaN; -0.0 passes
    live = ~skipped & ok
    v64 = (v + np.float32(0)).astype(np.float64)                          # -0.0 counts as 0
    scale = float(2 ** shift)
    q = np.rint(np.where(live, v64, 0.0) * scale).astype(np.int64)
    q2 = np.rint(np.where(live, v64, 0.0) * np.where(live, v64, 0.0) * scale).astype(np.int64)
    count, total, sq = (np.zeros(n_strata, dtype=np.int64) for _ in range(3))
    np.add.at(count, s[live], 1)
    np.add.at(total, s[live], q[live])
    np.add.at(sq, s[live], q2[live])
    return dict(count=count, sum=total, sumsq=sq, n_rows=int(live.sum()), n_rejected=int((~skipped & ~ok).sum()))


def moments_ref(ref, shift=32):
    """(mean, var) float64 of stats_ref's planes: sum / 2^shift / count and sumsq / 2^shift / count - mean^2 (not below 0), 0 where
    nothing landed."""
    count = ref["count"]
    div = np.maximum(count, 1).astype(np.float64)
    mean = np.where(count > 0, ref["sum"].astype(np.float64) / 2.0 ** shift / div, 0.0)
    var = np.where(count > 0, np.maximum(ref["sumsq"].astype(np.float64) / 2.0 ** shift / div - mean * mean, 0.0), 0.0)
    return mean, var


def table_ref(count, mean, var, mode, min_count):
    """float32 (offset, scale): 'logodds' offset = log(E) - log1p(-E), scale 1; 'ratio' offset 0, scale 1 / E; 'z' offset E, scale
    1 / sd.  count < min_count, E <= 0, (logodds) E >= 1 or (z) sd = 0: offset NaN, scale 1."""
    n = len(count)
    offset, scale = np.full(n, np.nan, dtype=np.float32), np.ones(n, dtype=np.float32)
    for s in range(n):
        E = float(mean[s])
        if count[s] < min_count or count[s] == 0 or not E > 0:
            continue
        if mode == "logodds":
            if E >= 1:
                continue
            offset[s] = np.float32(np.log(E) - np.log1p(-E))
        elif mode == "ratio":
            offset[s], scale[s] = np.float32(0), np.float32(1.0 / E)
        else:
            sd = float(np.sqrt(var[s]))
            if not sd > 0:
                continue
            offset[s], scale[s] = np.float32(E), np.float32(1.0 / sd)
    return offset, scale


def enrich_ref(score, strata, offset, scale):
    """float32 [n]: (score - offset[s]) * scale[s], each operation rounded to float32; NaN for stratum -1."""
    score = np.asarray(score, dtype=np.float32)
    s = np.asarray(strata)
    safe = np.where(s >= 0, s, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((score - offset[safe]).astype(np.float32) * scale[safe]).astype(np.float32)
    return np.where(s >= 0, out, np.float32(np.nan)).astype(np.float32)


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def reference_enrichment(rows, logit, k, edges, min_count, width=None):
    """What the reference's own logits give: (enrich float32 [n] by 'logodds', strata, offset, mean, count).  The expectation is the
    restatement's, fed float32(sigmoid(logit)) as the device would be."""
    value = sigmoid64(logit).astype(np.float32)
    ref = stats_ref(rows, value, k, edges)
    mean, var = moments_ref(ref)
    offset, scale = table_ref(ref["count"], mean, var, "logodds", min_count)
    s = strata_ref(rows, k, edges)
    return enrich_ref(np.asarray(logit, dtype=np.float32), s, offset, scale), s, offset, mean, ref["count"]


def best_cut(enrich, lo=10, hi=50):
    """(K, gap): the K in [lo, hi) with the largest gap between the K-th and the (K+1)-th best enrichment (NaN never ranks)."""
    e = np.sort(np.asarray(enrich, dtype=np.float64)[~np.isnan(enrich)])[::-1]
    best, gap = None, -1.0
    for K in range(lo, min(hi, len(e))):
        if e[K - 1] - e[K] > gap:
            best, gap = K, float(e[K - 1] - e[K])
    return best, gap


def enrich_tolerance(mean, kept, TOL=1e-4):
    """TOL (1 + 0.25 / min_s E_s (1 - E_s)) over the kept strata: the device's logit is within TOL of the reference's, a probability
    moves at most a quarter of that (d sigmoid <= 1/4), so does a stratum mean, and d logit(E) / dE = 1 / (E (1 - E))."""
    E = np.asarray(mean)[kept]
    return TOL * (1.0 + 0.25 / float(np.min(E * (1.0 - E))))
