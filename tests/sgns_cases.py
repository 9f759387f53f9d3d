"""Inputs on which sgns_kernel's one-launch result is THE sequential twin's (tests/walk_ref.py) although a position has several contexts, a
window above 1, its own centre among the draws or bad ids in reach: shared by tests/test_cpu_walk.py, which proves from
the twin alone the conditions each comparison rests on, and tests/test_hip_walk.py, which makes the comparisons.

Every builder returns (walks int32 [W, Lw], noise_cum int64 [N + 1], syn0, syn1 float32 [N + 1, d], kwargs of walk_ref.sgns /
walk.sgns_epoch); N = 5000.  The seeds were searched on the CPU for the conditions the tests assert from ``trained`` (walk_ref.draws)."""
import functools
import types

import numpy as np

from tests import walk_ref as WR

N = 5000
WIDTHS = (64, 128, 256)
DTYPES = ((np.float64, "seq"), (np.float32, "seq"), (np.float32, "tree"))
# dead flanks: the two constructed columns, in another lane and (d > 64) another register k of the kernel's k * 64 + lane mapping per width
AXES = {64: (17, 41), 128: (70, 101), 256: (131, 250)}
SEED_A1, SEED_A2, SEED_B, SEED_C = 1, 600, 2, 18


def tables(d, seed=0):
    rng = np.random.default_rng(100 + seed)
    return (rng.uniform(-0.5, 0.5, size=(N + 1, d)).astype(np.float32), rng.uniform(-0.5, 0.5, size=(N + 1, d)).astype(np.float32))


def _noise(weights):
    """The cumulative table of integer weights proportional to ``weights`` [N + 1] (row 0 is no node), summing to about 2^32."""
    w = np.asarray(weights, dtype=np.float64)
    w[0] = 0
    return np.cumsum(np.rint(2.0 ** 32 * w / w.sum()).astype(np.int64))


def trained(walks, noise_cum, epoch=0, n_nodes=None, *, window, negative, seed, epochs=1, **_):
    """The (centre, context) pairs a pass trains, in the twin's order, from the integer side alone: a list of (w, i, j, centre, context, b,
    the context's ``negative`` draws).  ``n_nodes``: the kernel's rule for ids outside 1 .. n_nodes."""
    W, Lw = walks.shape
    b_all, neg_all = WR.draws(W, Lw, epoch * W * Lw, noise_cum, window, negative, seed)
    out = []
    for w in range(W):
        for i in range(Lw):
            centre, b = int(walks[w, i]), int(b_all[w * Lw + i])
            if n_nodes is not None and not 1 <= centre <= n_nodes:
                continue
            for j in range(max(0, i - b), min(Lw - 1, i + b) + 1):
                ctx = int(walks[w, j])
                if j == i or (n_nodes is not None and not 1 <= ctx <= n_nodes):
                    continue
                out.append((w, i, j, centre, ctx, b, neg_all[w * Lw + i, j - (i - window)].tolist()))
    return out


def twins(walks, syn0, syn1, noise_cum, kw, epochs_run=(0,), n_nodes=None):
    """{(dtype, order): [the twin's (syn0, syn1) after each pass of ``epochs_run`` in turn]} for float64 and float32 in both orders."""
    out = {}
    for dtype, order in DTYPES:
        a, passes = (syn0, syn1), []
        for ep in epochs_run:
            a = WR.sgns(walks, a[0], a[1], noise_cum, epoch=ep, dtype=dtype, order=order, n_nodes=n_nodes, **kw)
            passes.append(a)
        out[(dtype, order)] = passes
    return out


# ---- A: several live contexts per position ("dead flanks") -------------------------------------------------------------------------------
def dead_flanks(d, centres_in_noise=False):
    """8 walks [x, c, y] over 24 distinct ids, window 1.  The middle position (centre c, contexts x and y) is the only one that moves
    anything: u carries from x to y and neu restarts.  The flanks (centre x or y, context c) are built to contribute exact zeros through two
    reserved columns E1, E2 = AXES[d]: syn0 is 0 there but syn0[c] = 12; syn1[:, E1] = -10 (every row a sink for v = syn0[c]) but
    syn1[x, E1] = syn1[y, E1] = 4 and syn1[c] = (0, -10) on (E1, E2).  A flank's positive dot is 48 + O(1): 1 - sigmoid is exactly 0 in
    float32 and float64; its negatives' dots are -120 + O(1): expf(-f) = +inf and g_t = 0 in float32 (1e-53 in float64).  Whatever order the
    flanks' atomics arrive in, they add zeros to what the middle reads and writes.  The middle's dots stay moderate (syn0[x], syn0[y] are
    0 on both columns).

    ``centres_in_noise`` (A2, run one walk per launch): the noise table weighs a sink 1, a centre c 400, x and y 0 -- a middle draws its own
    centre (skipped) and other walks' centres (live rows, but of another launch)."""
    rng = np.random.default_rng(7)
    walks = rng.choice(np.arange(1, N + 1), size=24, replace=False).reshape(8, 3).astype(np.int32)
    x, c, y = walks[:, 0], walks[:, 1], walks[:, 2]
    e1, e2 = AXES[d]
    syn0, syn1 = tables(d, 2)
    syn0[:, [e1, e2]] = 0
    syn1[:, e1], syn1[:, e2] = -10, 0
    syn1[x, e1] = syn1[y, e1] = 4
    syn1[c, e1], syn1[c, e2] = 0, -10
    syn0[c, e1] = syn0[c, e2] = 12
    wts = np.ones(N + 1)
    wts[walks.ravel()] = 0
    if centres_in_noise:
        wts[c] = 400
        kw = dict(window=1, negative=5, lr0=0.1, lr1=1e-4, seed=SEED_A2, epochs=4)
    else:
        kw = dict(window=1, negative=5, lr0=0.1, lr1=1e-4, seed=SEED_A1, epochs=2)
    return walks, _noise(wts), syn0, syn1, kw


def free_columns(d):
    """The columns the dead flanks' grade is taken over: all but the constructed two (their 10 to 12 would loosen max|r| about 24-fold)."""
    cols = np.ones(d, dtype=bool)
    cols[list(AXES[d])] = False
    return cols


def flank_margins(walks, syn0, syn1, pairs):
    """(the smallest positive dot, the largest negative dot) over the flank positions of ``pairs`` (of ``trained``), in float64."""
    s0, s1 = np.asarray(syn0, dtype=np.float64), np.asarray(syn1, dtype=np.float64)
    pos, neg = [], []
    for w, i, j, centre, ctx, b, ids in pairs:
        if i != 1:
            pos.append(float(s0[ctx] @ s1[centre]))
            neg += (s1[[t for t in ids if t != centre]] @ s0[ctx]).tolist()
    return min(pos), max(neg)


# ---- B: the negatives' stream slot jj at window > 1 -----------------------------------------------------------------------------------
def wide_window(d):
    """The race-free shape of tests/test_hip_walk.py (8 walks of length 2 over 16 distinct ids, a noise table off them) at window 5: b is
    drawn from 1 .. 5, the one context is always in reach, and the negatives come from slot jj = window + 1 or window - 1."""
    rng = np.random.default_rng(3)
    walks = rng.choice(np.arange(1, N + 1), size=16, replace=False).reshape(8, 2).astype(np.int32)
    wts = np.ones(N + 1)
    wts[walks.ravel()] = 0
    return (walks, _noise(wts)) + tables(d, 3) + (dict(window=5, negative=5, lr0=0.025, lr1=1e-4, seed=SEED_B, epochs=1),)


# ---- C: the window draw, clipping at the walk's ends, bad ids among the contexts -----------------------------------------------------------
C_PLACES = [(p, dist) for dist in (1, 2, 3) for p in (0, (5 - dist) // 2, 5 - dist)]        # the pair at the start, mid-walk, at the end


def clipped_pairs(d):
    """18 walks of length 6 at window 3, each with exactly two valid ids, at (p, p + dist) for every place of C_PLACES twice; the other
    four slots hold 0 or N + 1, mixed.  A position trains its partner iff its b >= dist; the bad slots in reach are skipped and flagged.
    All valid ids are distinct and off the noise table: two positions never meet in a row."""
    rng = np.random.default_rng(11)
    ids = rng.choice(np.arange(1, N + 1), size=36, replace=False).reshape(18, 2)
    walks = np.zeros((18, 6), dtype=np.int32)
    for w, (p, dist) in enumerate(C_PLACES + C_PLACES):
        walks[w] = [0 if (w // 9 + s) % 2 == 0 else N + 1 for s in range(6)]
        walks[w, p], walks[w, p + dist] = ids[w]
    wts = np.ones(N + 1)
    wts[ids.ravel()] = 0
    return (walks, _noise(wts)) + tables(d, 4) + (dict(window=3, negative=5, lr0=0.1, lr1=1e-4, seed=SEED_C, epochs=1),)


# ---- the four cases as the tests run them -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, d):
    """Case ``name`` at width d with its three twins, computed once and shared (the arrays are read-only): A1 = the dead flanks in one launch,
    passes 0 and 1 of 2; A2 = the dead flanks with the centres in the noise table, pass 1 of 4 (so g_base has an epoch's and a walk's
    part), one walk per launch; B = wide_window, C = clipped_pairs, one pass in one launch."""
    build, args, epochs_run, n_nodes = {"A1": (dead_flanks, (d,), (0, 1), None), "A2": (dead_flanks, (d, True), (1,), None),
                                        "B": (wide_window, (d,), (0,), None), "C": (clipped_pairs, (d,), (0,), N)}[name]
    walks, noise, syn0, syn1, kw = build(*args)
    for a in (walks, noise, syn0, syn1):
        a.flags.writeable = False
    c = types.SimpleNamespace(name=name, d=d, walks=walks, noise=noise, syn0=syn0, syn1=syn1, kw=kw, epochs_run=epochs_run, n_nodes=n_nodes,
                              cols=free_columns(d) if name in ("A1", "A2") else np.ones(d, dtype=bool))
    c.trained = [trained(walks, noise, ep, n_nodes, **kw) for ep in epochs_run]
    c.twins = twins(walks, syn0, syn1, noise, kw, epochs_run, n_nodes)
    return c


def noise_floor(c, p=-1):
    """Per table (syn0, syn1) the grade's noise term after pass ``p`` of the case: max(e(R32 seq), e(R32 tree), 2^-23) against the float64
    twin over the case's columns (tests/fp64_grade.py)."""
    from tests.fp64_grade import ULP, tensor_err
    r64, ra, rb = (c.twins[k][p] for k in DTYPES)
    return [max(tensor_err(a[:, c.cols], r[:, c.cols]), tensor_err(b[:, c.cols], r[:, c.cols]), ULP) for r, a, b in zip(r64, ra, rb)]
