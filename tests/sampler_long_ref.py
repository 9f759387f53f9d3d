"""Plain-Python twin of matcha_neg_sample_long (matcha_amd/csrc/sampler.hip, neg_sample_long_kernel) -- TEST INFRASTRUCTURE.

oracle/sampler.py restates the sampler for rows of up to 8 columns and draws replacement p of trial t at counter 8*t + p.  Rows of up to
32 columns need another stride (at stride 8, position 8 of trial t would reuse the draw of position 0 of trial t + 1), so this file states
the rule of include/matcha_hip.h on the same counter RNG (oracle/rng.py, STREAM_NEG):

    key               make_key(seed, STREAM_NEG); the hi counter is the negative's index n = neg_num*j + i
    mask              rand(key, n, 0xFFFF0000 + a) & (2^k - 1), redrawn (a = 0, 1, ...) while zero; for k = 32 all 32 bits
    replacement       rand(key, n, S*trial + position),  S = 8 when L <= 8,  S = 32 when L > 8;  32*65535 + 31 < 0xFFFF0000
    value             start + floor(r * (end - start) / 2^32) in the chromosome of the node it replaces (main.py:405-407)

and the accept / reject rules of generate_negative (main.py:383-428) exactly as oracle/sampler.py states them.  At L <= 8 the two files
must agree bit for bit (tests/test_cpu_long_sampler.py).  A chosen node outside [1, n_nodes] or without a chromosome is kept and
flagged in status[0] (bit 2); a negative whose 65 536 trials are exhausted is returned equal to its positive and counted in status[1].
"""
import numpy as np

from oracle import rng as R

MAX_TRIALS = 1 << 16
MAX_LONG_L = 32
STATUS_BAD_CHROM = 2


def stride_of(L: int) -> int:
    return 8 if L <= 8 else 32


def sample_negatives_long(pos, known, node2chrom, chrom_range, neg_num, min_dis, seed, return_status=False):
    """pos int64 [P, L] zero-padded ascending rows, L <= 32; ``known`` = set of tuples (without padding).
    Returns int64 [P*neg_num, L] (and the status word int32 [4] when asked): negatives of positive j at rows neg_num*j ..."""
    pos = np.asarray(pos, dtype=np.int64)
    P, L = pos.shape
    assert 1 <= L <= MAX_LONG_L
    S = stride_of(L)
    n_nodes = len(node2chrom) - 1
    n_chrom = len(chrom_range)
    out = np.zeros((P * neg_num, L), dtype=np.int64)
    status = np.zeros(4, dtype=np.int32)
    key = R.make_key(seed, R.STREAM_NEG)
    for j in range(P):
        nzp = np.nonzero(pos[j])[0]
        k = int(nzp[-1]) + 1 if len(nzp) else 0                       # index of the last non-zero + 1
        orig = [int(v) for v in pos[j, :k]]
        for i in range(neg_num):
            n = j * neg_num + i
            result = list(orig)
            if len(known) > 0 and k > 0 and tuple(orig) in known:       # main.py:390-392: entered only if the positive is a member
                kmask = 0xFFFFFFFF if k >= 32 else (1 << k) - 1
                mask, a = 0, 0
                while mask == 0:
                    mask = int(R.rand_u32(key, n, 0xFFFF0000 + a)) & kmask
                    a += 1
                chosen = [p_ for p_ in range(k) if (mask >> p_) & 1]
                start, length, redraw = [], [], []
                for p_ in chosen:
                    v = orig[p_]
                    c = int(node2chrom[v]) if 1 <= v <= n_nodes else -1
                    if 0 <= c < n_chrom:
                        redraw.append(p_)
                        start.append(int(chrom_range[c][0]))
                        length.append(int(chrom_range[c][1]) - int(chrom_range[c][0]))
                    else:
                        status[0] |= STATUS_BAD_CHROM                  # kept as it is, flagged
                lo = np.asarray(redraw, dtype=np.uint64)
                done = False
                for trial in range(MAX_TRIALS):
                    cand = list(orig)
                    if redraw:
                        r = R.rand_u32(key, n, np.uint64(S * trial) + lo)
                        for t, p_ in enumerate(redraw):
                            cand[p_] = start[t] + ((int(r[t]) * length[t]) >> 32)
                    cand.sort()
                    if any((cand[t + 1] - cand[t]) == 0 or (cand[t + 1] - cand[t]) <= min_dis for t in range(k - 1)):
                        continue
                    if tuple(cand) in known:
                        continue
                    result, done = cand, True
                    break
                if not done:
                    status[1] += 1
            out[n, :k] = result
    return (out, status) if return_status else out


def check_invariants(pos, neg, known, node2chrom, neg_num, min_dis):
    """Every invariant of SURVEY.md section 8 c3 on the negatives of KNOWN positives: same k as the positive, ascending and duplicate-free,
    gaps > min_dis, not known, the same chromosome multiset, at least one node changed.  Returns the number of negatives checked."""
    n2c = np.asarray(node2chrom)
    checked = 0
    for n in range(len(neg)):
        p = pos[n // neg_num]
        k = int((p != 0).sum())
        r = neg[n]
        assert (r[k:] == 0).all() and (r[:k] != 0).all(), (n, p, r)
        p, r = p[:k], r[:k]
        if tuple(p.tolist()) not in known:
            assert np.array_equal(p, r), (n, p, r)                     # not a member: copied
            continue
        assert (np.diff(r) > min_dis).all(), (n, r)
        assert tuple(r.tolist()) not in known, (n, r)
        assert sorted(n2c[r].tolist()) == sorted(n2c[p].tolist()), (n, p, r)
        assert not np.array_equal(p, r), (n, p)
        checked += 1
    return checked


def statistics(batch, neg, neg_num, ks):
    """Per k in ``ks``: (histogram of the number of nodes a negative differs from its positive in, histogram of WHICH position of the
    positive was replaced) -- what tests/golden/make_golden_long_sampler.py took on the reference's generate_negative."""
    diff = {k: np.zeros(k + 1, dtype=np.int64) for k in ks}
    posh = {k: np.zeros(k, dtype=np.int64) for k in ks}
    for n in range(len(neg)):
        p = batch[n // neg_num]
        k = int((p != 0).sum())
        rs = set(neg[n, :k].tolist())
        gone = [i for i in range(k) if int(p[i]) not in rs]
        diff[k][len(gone)] += 1
        for i in gone:
            posh[k][i] += 1
    return diff, posh


def chi2_two_sample(a, b):
    """Two-sample chi-square of two histograms, sum (sqrt(B/A) a - sqrt(A/B) b)^2 / (a + b) with A, B the totals -- for equal totals (the
    differing-node histograms) this is sum (a - b)^2 / (a + b) as in tests/helpers.c3_chi2_against_reference; the replaced-position
    histograms' totals differ by the sampling noise of how many nodes were replaced -- after pooling every bin whose two counts together
    are below 10 into one.  Returns (statistic, bins used)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    small = (a + b) < 10
    aa, bb = list(a[~small]), list(b[~small])
    if small.any() and (a[small].sum() + b[small].sum()) > 0:
        aa.append(a[small].sum())
        bb.append(b[small].sum())
    aa, bb = np.asarray(aa), np.asarray(bb)
    ra, rb = np.sqrt(bb.sum() / aa.sum()), np.sqrt(aa.sum() / bb.sum())
    return float((((ra * aa - rb * bb) ** 2) / (aa + bb)).sum()), len(aa)


def long_sampler_case(min_dis, ks=(9, 12, 16, 25), per_k=2000, batch_per_k=1000):
    """The positives sampler_stats_long.npz was taken on: hg38 1 Mb, ``per_k`` distinct hyperedges per k with all adjacent gaps > min_dis
    (otherwise the reference never returns), the first ``batch_per_k`` of each k as ONE shuffled mixed-k batch zero-padded to L = 25.
    Returns (batch int64 [P, 25], known = {tuple without padding}, all known rows padded [M, 25])."""
    from matcha_amd import synth
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    L = max(ks)
    rng = np.random.default_rng(130 + min_dis)
    pos_by_k = {}
    for k in ks:
        v = synth.make_edges_fast(rng, N, k, 3 * per_k)
        v = v[(np.diff(v, axis=1) > min_dis).all(axis=1)]
        assert len(v) >= per_k, (k, len(v))
        pos_by_k[k] = v[:per_k]
    rows = [np.pad(r, (0, L - k)) for k in ks for r in pos_by_k[k][:batch_per_k]]
    order = np.random.default_rng(177).permutation(len(rows))
    batch = np.stack([rows[o] for o in order]).astype(np.int64)
    known_rows = np.concatenate([np.pad(v, ((0, 0), (0, L - k))) for k, v in pos_by_k.items()]).astype(np.int64)
    known = {tuple(int(t) for t in r if t != 0) for r in known_rows}
    return batch, known, known_rows
