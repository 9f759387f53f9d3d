"""Plain-Python twin of matcha_outlier_plant (matcha_amd/csrc/sampler.hip, outlier_plant_kernel) and of the order rule of
matcha_locus_scores (matcha_amd/csrc/locus.hip, head_scores_kernel) -- TEST INFRASTRUCTURE.

The plant rule, as include/matcha_hip.h states it, on the counter RNG of oracle/rng.py with the stream id 18 (STREAM_OUTLIER):

    row         local row i of a call is global row n = n0 + i, a copy of positive i // draws (copy n % draws where draws divides n0)
    k           the positive's non-zero prefix
    position    p = (n % draws) % k with cycle, else (rand(key, n, 0xFFFF0000) * k) >> 32
    trial t     0 .. 255: j = start + ((rand(key, n, t) * (end - start)) >> 32) in the chromosome of the positive's locus p;
                cand = the positive without locus p plus j, ascending.  Refused: j is a locus of the positive; an adjacent gap <= min_dis;
                (pairs given) a pair (min(j, v), max(j, v)), v another locus of cand, is known; (known given) cand is known
    out         cand zero-padded, planted = the index of j in cand

No plant -- trials exhausted, k < 2, a locus outside [1, n_nodes], locus p without a chromosome (node2chrom outside [0, n_chrom), or an empty
range): a copy of the positive, planted = -1; status[0] |= 2 for the last two, status[1] counts the rows whose 256 trials were exhausted.

The order rule: the slots of a row's real loci ascending by score, ties to the lower slot, a NaN behind every number; -1 behind the k-th.
"""
import numpy as np

from oracle import rng as R

STREAM_OUTLIER = 18
PLANT_TRIALS = 256
STATUS_BAD_CHROM = 2


def plant_outliers(pos, known, pairs, node2chrom, chrom_range, draws, cycle, min_dis, seed, n0=0):
    """pos int64 [P, L] zero-padded ascending rows; ``known`` = set of tuples (without padding) or empty; ``pairs`` = set of (lo, hi) or
    empty.  Returns (rows int64 [P*draws, L], planted int32 [P*draws], status int32 [4])."""
    pos = np.asarray(pos, dtype=np.int64)
    P, L = pos.shape
    assert 1 <= L <= 32 and draws >= 1 and n0 >= 0
    n_nodes, n_chrom = len(node2chrom) - 1, len(chrom_range)
    out = np.zeros((P * draws, L), dtype=np.int64)
    planted = np.full(P * draws, -1, dtype=np.int32)
    status = np.zeros(4, dtype=np.int32)
    key = R.make_key(seed, STREAM_OUTLIER)
    for i in range(P * draws):
        n = n0 + i
        row = pos[i // draws]
        zeros = np.nonzero(row == 0)[0]
        k = int(zeros[0]) if len(zeros) else L
        orig = [int(v) for v in row[:k]]
        out[i] = row
        if any(not (1 <= v <= n_nodes) for v in orig):
            status[0] |= STATUS_BAD_CHROM
            continue
        if k < 2:
            continue
        p = (n % draws) % k if cycle else (int(R.rand_u32(key, n, 0xFFFF0000)) * k) >> 32
        c = int(node2chrom[orig[p]])
        start, length = 0, 0
        if 0 <= c < n_chrom:
            start, length = int(chrom_range[c][0]), int(chrom_range[c][1]) - int(chrom_range[c][0])
        if length <= 0:
            status[0] |= STATUS_BAD_CHROM
            continue
        rest = orig[:p] + orig[p + 1:]
        r = R.rand_u32(key, n, np.arange(PLANT_TRIALS, dtype=np.uint64))
        done = False
        for t in range(PLANT_TRIALS):
            j = start + ((int(r[t]) * length) >> 32)
            if j in orig:
                continue
            cand = sorted(rest + [j])
            if any(cand[q + 1] - cand[q] == 0 or cand[q + 1] - cand[q] <= min_dis for q in range(k - 1)):
                continue
            if pairs and any((min(j, v), max(j, v)) in pairs for v in cand if v != j):
                continue
            if known and tuple(cand) in known:
                continue
            out[i, :k] = cand
            planted[i] = cand.index(j)
            done = True
            break
        if not done:
            status[1] += 1
    return out, planted, status


def lowest_order(scores, x, lowest):
    """int64 [B, lowest]: the order rule applied to ``scores`` [B, L] of the rows ``x`` [B, L] (a slot is real where x != 0)."""
    scores, x = np.asarray(scores, dtype=np.float32), np.asarray(x)
    B, L = x.shape
    order = np.full((B, lowest), -1, dtype=np.int64)
    for b in range(B):
        slots = [l for l in range(L) if x[b, l] != 0]
        # python's sort is stable: slots ascending on equal keys; (is NaN, value) puts a NaN behind every number, and -0.0 == 0.0
        slots.sort(key=lambda l: (1, 0.0) if np.isnan(scores[b, l]) else (0, float(scores[b, l])))
        m = min(lowest, len(slots))
        order[b, :m] = slots[:m]
    return order


def hits_recount(order, planted, sizes, top):
    """{s: (rows, [hits at rank r for r < top])} for s in 2 .. 32 -- what matcha_amd.outlier.outlier_hits counts, recounted with numpy:
    a row is valid when planted >= 0, and hits rank r when order[:, r] == planted."""
    order, planted, sizes = np.asarray(order), np.asarray(planted), np.asarray(sizes)
    res = {}
    for s in range(2, 33):
        sel = (sizes == s) & (planted >= 0)
        hits = [int((order[sel, r] == planted[sel]).sum()) if r < order.shape[1] else 0 for r in range(top)]
        res[s] = (int(sel.sum()), hits)
    return res


def plant_case(layout, L, min_dis, P=37, seed=0):
    """The positives and sets the plant tests share: (num, pos int64 [P, L], known tuples, known rows [M, L], pairs {(lo, hi)}, pair rows
    [Q, 2]).  Sizes 2, 3, min(L, 5) and the widest that fits -- L itself on the large layouts, at most 8 on the 64-node tiny one -- all
    adjacent gaps > min_dis (otherwise no plant can pass the gap rule); every other pool row is a known hyperedge, and every pair inside
    the first pool rows of each size a known pair, so that both set refusals are met on the way."""
    from matcha_amd import synth
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(1900 + 37 * L + min_dis + seed)
    ks = sorted({2, 3, min(L, 5), min(L, 8) if layout == "tiny" else L})
    pools = []
    for k in ks:
        v = synth.make_edges_fast(rng, N, k, 400)
        v = v[(np.diff(v, axis=1) > min_dis).all(axis=1)][:60]
        assert len(v) >= 10, (layout, L, k, len(v))
        pools.append(np.pad(v, ((0, 0), (0, L - k))))
    pos = np.stack([pools[i % len(pools)][i // len(pools)] for i in range(P)]).astype(np.int64)
    pool = np.concatenate(pools).astype(np.int64)
    known_rows = pool[::2]
    known = {tuple(int(t) for t in r if t) for r in known_rows}
    pairs = set()
    for p_ in pools:
        for r in p_[:12]:
            v = [int(t) for t in r if t]
            pairs |= {(a, b) for ia, a in enumerate(v) for b in v[ia + 1:]}
    pair_rows = np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    return num, pos, known, known_rows, pairs, pair_rows


def check_plant_invariants(pos, rows, planted, known, pairs, node2chrom, draws, min_dis):
    """Every invariant of a planted row against its positive; returns the number of planted rows checked."""
    n2c = np.asarray(node2chrom)
    checked = 0
    for i in range(len(rows)):
        p_, r_ = pos[i // draws], rows[i]
        k = int((p_ != 0).sum())
        assert (r_[k:] == 0).all() and (r_[:k] != 0).all(), (i, p_, r_)
        p_, r_ = p_[:k].tolist(), r_[:k].tolist()
        if planted[i] < 0:
            assert p_ == r_, (i, p_, r_)
            continue
        assert all(b - a > max(min_dis, 0) for a, b in zip(r_, r_[1:])), (i, r_)            # ascending, duplicate-free, gaps > min_dis
        assert not known or tuple(r_) not in known, (i, r_)
        j = r_[planted[i]]
        assert j not in p_, (i, p_, r_)                                                     # planted indexes the new locus
        assert len(set(p_) - set(r_)) == 1 and len(set(r_) - set(p_)) == 1, (i, p_, r_)     # exactly one locus differs
        assert not pairs or not any((min(j, v), max(j, v)) in pairs for v in r_ if v != j), (i, r_)
        assert sorted(n2c[r_].tolist()) == sorted(n2c[p_].tolist()), (i, p_, r_)
        checked += 1
    return checked
