"""Cluster growth restated in plain Python with sets, on top of tests/complete_ref.py: the twin of csrc/grow.hip's two
kernels and of matcha_amd/sweep.py's grow_step and growth_sweep.  No GPU, no torch; tests/test_cpu_grow.py and tests/test_hip_grow.py
both check against it, and tests/golden/make_golden_grow.py drives the reference with it.

The rule.  A beam is [A][B] slots, every slot a cluster row of 7.10 (the leading non-zero run).  One step adds one bin of [lo, lo + n) to
every slot: candidate (a, j, r) is 7.10's candidate of slot j of seed a with the free id lo + r; its rank within the seed is j n + r.
It is a TWIN iff some lower slot j' < j of the seed is strictly ascending, non-empty, holds as many ids as slot j -- which must be
strictly ascending too -- and set(slot_j') <= set(slot_j) | {lo + r}.  Per seed the best K = min(beam, B n) candidates that are valid,
not twins and not excluded are kept: higher score first, then lower rank; a NaN score is never kept.  The score function is the caller's."""
import numpy as np

from tests import complete_ref as CR


def strict(ids):
    return all(a < b for a, b in zip(ids, ids[1:]))


def related(u, v):
    """Slot u (lower) can make a candidate of slot v a twin at all."""
    return len(u) >= 1 and len(u) == len(v) and strict(u) and strict(v)


def is_twin(slots, j, new_id):
    """Is the candidate (slot j, new_id) of one seed's slots a twin."""
    v = CR.leading_ids(slots[j])
    return any(related(u, v) and set(u) <= set(v) | {new_id} for u in (CR.leading_ids(s) for s in slots[:j]))


def twin_table(beam):
    """int64 [A B, B] of a beam [A][B][S]: what matcha_grow_twins writes.  Column j' < j of row a B + j: the one id of slot_j' \\ slot_j,
    -1 for identical slots, 0 for no relation (different sizes, more than one id apart, an empty or not strictly ascending slot)."""
    beam = np.asarray(beam, dtype=np.int64)
    A, B, _ = beam.shape
    out = np.zeros((A * B, B), dtype=np.int64)
    for a in range(A):
        ids = [CR.leading_ids(s) for s in beam[a]]
        for j in range(B):
            for jp in range(j):
                if related(ids[jp], ids[j]):
                    extra = set(ids[jp]) - set(ids[j])
                    out[a * B + j, jp] = -1 if not extra else extra.pop() if len(extra) == 1 else 0
    return out


def twin_flags(beam, lo, n):
    """bool [A B n] in global-rank order, straight from the set rule (not from twin_table)."""
    beam = np.asarray(beam, dtype=np.int64)
    A, B, _ = beam.shape
    return np.asarray([is_twin(beam[a], j, lo + r) for a in range(A) for j in range(B) for r in range(n)], dtype=bool).reshape(A * B * n)


def candidates(beam, lo, n, min_gap, width):
    """(rows int64 [A B n, width], invalid bool, twin bool) of a beam in global-rank order."""
    beam = np.asarray(beam, dtype=np.int64)
    A, B, S = beam.shape
    rows, bad = CR.table(beam.reshape(A * B, S), lo, n, 1, min_gap, width)
    return rows, bad, twin_flags(beam, lo, n)


def select(scores, skip, A, seg, K):
    """Per segment of ``seg`` consecutive ranks the best K (higher score, then lower rank) of the rows with skip == False and a score
    that is not NaN: int64 [A, K] of ranks WITHIN the segment, -1 behind the kept ones."""
    scores = np.asarray(scores)
    out = np.full((A, K), -1, dtype=np.int64)
    for a in range(A):
        sc = scores[a * seg:(a + 1) * seg]
        ok = [i for i in range(seg) if not skip[a * seg + i] and not np.isnan(sc[i])]
        ok.sort(key=lambda i: (-float(sc[i]), i))
        out[a, :min(K, len(ok))] = ok[:K]
    return out


def step(beam, lo, n, min_gap, width, beam_out, score, excluded=None):
    """One step.  ``score(rows) -> float array [len(rows)]``; ``excluded(rows) -> bool array`` or None.  Returns a dict of numpy arrays:
    rows [A, K, width], logit [A, K] (the score's dtype), rank, parent, added [A, K], count [A], beam [A, K, S + 1], and the integers
    n_candidates, n_invalid, n_twins (valid candidates that are twins), n_excluded (valid, non-twin candidates that are excluded)."""
    beam = np.asarray(beam, dtype=np.int64)
    A, B, S = beam.shape
    K = min(beam_out, B * n)
    rows, bad, tw = candidates(beam, lo, n, min_gap, width)
    logits = np.asarray(score(rows)).reshape(-1)
    skip = bad | tw
    n_exc = 0
    if excluded is not None:
        known = np.asarray(excluded(rows), dtype=bool)
        n_exc = int((known & ~skip).sum())
        skip = skip | known
    rank = select(logits, skip, A, B * n, K)
    kept = rank >= 0
    g = np.where(kept, rank + np.arange(A).reshape(-1, 1) * (B * n), 0)
    out_rows = np.where(kept[..., None], rows[g], 0)
    return {"rows": out_rows, "logit": np.where(kept, logits[g], 0).astype(logits.dtype), "rank": rank, "parent": np.where(kept, rank // n, 0),
            "added": np.where(kept, lo + rank % n, 0), "count": kept.sum(axis=1), "beam": out_rows[:, :, :S + 1].copy(),
            "n_candidates": A * B * n, "n_invalid": int(bad.sum()), "n_twins": int((tw & ~bad).sum()), "n_excluded": n_exc}


def grow(seeds, lo, n, max_size, beam, min_gap, width, score, excluded=None):
    """The whole growth of ``seeds`` (id lists; sorted here): growth_sweep's arrays rows [A, T, B, width], logit, parent, added
    [A, T, B], count, size [A, T], path [A, B, T] and its integers."""
    seeds = [sorted(int(v) for v in s if int(v) != 0) for s in seeds]
    A, B = len(seeds), beam
    sizes = [len(s) for s in seeds]
    some = [s for s in sizes if s >= 1]
    T = max(max_size - min(some), 0) if some else 0
    levels = [max_size - s if 1 <= s < max_size else 0 for s in sizes]
    out = {"rows": np.zeros((A, T, B, width), dtype=np.int64), "logit": np.zeros((A, T, B), dtype=np.float32),
           "parent": np.zeros((A, T, B), dtype=np.int64), "added": np.zeros((A, T, B), dtype=np.int64),
           "count": np.zeros((A, T), dtype=np.int64), "size": np.zeros((A, T), dtype=np.int64), "path": np.zeros((A, B, T), dtype=np.int64)}
    tot = {"n_candidates": 0, "n_invalid": 0, "n_twins": 0, "n_excluded": 0, "steps": 0}
    if n < 1:
        return {**out, **tot}
    cur = {a: [seeds[a]] for a in range(A) if levels[a] > 0}
    for t in range(T):
        active = [a for a in cur if levels[a] > t]
        if not active:
            break
        S = max(sizes[a] for a in active) + t
        table = np.stack([CR.padded(cur[a], S) for a in active])
        res = step(table, lo, n, min_gap, width, B, score, excluded)
        K = res["rank"].shape[1]
        for i, a in enumerate(active):
            for key in ("rows", "logit", "parent", "added"):
                out[key][a, t, :K] = res[key][i]
            out["count"][a, t] = res["count"][i]
            out["size"][a, t] = sizes[a] + t + 1
            cur[a] = [CR.leading_ids(r) for r in res["beam"][i]]
        for key in ("n_candidates", "n_invalid", "n_twins", "n_excluded"):
            tot[key] += res[key]
        tot["steps"] += 1
    for a in range(A):
        for j in range(out["count"][a, levels[a] - 1] if levels[a] else 0):
            slot = j
            for t in range(levels[a] - 1, -1, -1):
                out["path"][a, j, t] = out["added"][a, t, slot]
                slot = out["parent"][a, t, slot]
    return {**out, **tot}


# ---- the g17 fixture (tests/golden/make_golden_grow.py) ---------------------------------------------------------------------------------
G17_CASES = [((1, 65), 4, 1, (1, 2, 3), 6, 8), ((17, 49), 4, 1, (1, 5, 9, 10), 13, 16), ((1, 65), 3, 2, (1, 3, 6), 7, 12),
             ((1, 65), 8, 1, (27, 29, 31), 32, 32)]              # (region, beam, min_gap, seed sizes, max_size, width)
G17_SEED = 1700
G17_TOL = 1e-4                                              # the project's tolerance against the reference's logits
G17_NEAR = 2                                                # at most this many candidates per (case, mode) within TOL of a B-th logit


def g17_seeds(case, n_nodes=64):
    """The seeds of one case, drawn the way complete_ref.g15_clusters draws its clusters: default_rng(G17_SEED + case)."""
    _, _, min_gap, sizes, _, _ = G17_CASES[case]
    rng = np.random.default_rng(G17_SEED + case)
    out = []
    for size in sizes:
        top = n_nodes - (size - 1) * (min_gap - 1)
        ids = np.sort(rng.choice(np.arange(1, top + 1), size=size, replace=False)) + np.arange(size) * (min_gap - 1)
        out.append([int(v) for v in ids])
    return out


def g17_steps(case):
    """[(t, active seed indices, B_t, S_t)] of one case: the steps its growth runs."""
    (lo, hi), B, _, sizes, max_size, _ = G17_CASES[case]
    n, out, B_t = hi - lo, [], 1
    for t in range(max_size - min(sizes)):
        active = [a for a, s in enumerate(sizes) if s + t < max_size]
        out.append((t, active, B_t, max(sizes[a] for a in active) + t))
        B_t = min(B, B_t * n)
    return out
