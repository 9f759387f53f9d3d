"""numpy twins of the hypergraph walk (csrc/walk.hip) and of the skip-gram pass (csrc/sgns.hip): the checkers of tests/test_cpu_walk.py and
tests/test_hip_walk.py.

* ``walks(graph, ...)`` -- the walk on a ``matcha_amd.walk.HyperWalkGraph``'s tables, vectorised over the walkers.  Integer arithmetic and
  the counter RNG of oracle/rng.py: equal to the kernel's output bit for bit.
* ``sgns(...)`` -- the skip-gram pass position by position in sequence (the kernel runs all positions at once and meets in the tables
  through float atomics: equal only where no two positions touch one row), in float64, or in float32 with the dot products summed
  in one of two orders.
"""
import numpy as np

from oracle import rng as R

STREAM_WALK, STREAM_SGNS = 19, 20
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def mulhi64(a, b):
    """floor(a b / 2^64) of uint64 arrays."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    al, ah, bl, bh = a & _M32, a >> _S32, b & _M32, b >> _S32
    p0, p1, p2, p3 = al * bl, ah * bl, al * bh, ah * bh
    mid = (p0 >> _S32) + (p1 & _M32) + (p2 & _M32)
    return p3 + (p1 >> _S32) + (p2 >> _S32) + (mid >> _S32)


def rand_u64(key, hi, lo):
    lo = np.asarray(lo, dtype=np.uint64)
    return (R.rand_u32(key, hi, lo).astype(np.uint64) << _S32) | R.rand_u32(key, hi, lo + np.uint64(1)).astype(np.uint64)


def cum_draw(cum, begin, count, u):
    """Per element the first i in [0, count) with cum[begin + i] > mulhi64(u, cum[begin + count - 1]) (count >= 1)."""
    begin, count = np.asarray(begin, dtype=np.int64), np.asarray(count, dtype=np.int64)
    r = mulhi64(u, cum[begin + count - 1])
    lo, hi = np.zeros_like(begin), count - 1
    while np.any(lo < hi):
        mid = (lo + hi) >> 1
        right = cum[begin + mid] > r
        go = lo < hi
        hi = np.where(go & right, mid, hi)
        lo = np.where(go & ~right, mid + 1, lo)
    return lo


class Tables:
    """A HyperWalkGraph's tables as numpy arrays."""

    def __init__(self, graph):
        self.N = graph.n_nodes
        self.ptr = graph.inc_ptr.cpu().numpy().astype(np.int64)
        self.nb = graph.inc_nb.cpu().numpy().astype(np.int64)
        self.cum = graph.inc_cum.cpu().numpy().astype(np.uint64)
        B = np.int64(self.N + 1)
        pr, tr = graph.pairs.cpu().numpy().astype(np.int64), graph.triples.cpu().numpy().astype(np.int64)
        self.pair_keys = np.sort(pr[:, 0] * B + pr[:, 1])
        self.triple_keys = np.sort((tr[:, 0] * B + tr[:, 1]) * B + tr[:, 2])
        self.thr = np.asarray(graph.thresholds, dtype=np.uint64)

    def classes(self, src, dst, c):
        B = np.int64(self.N + 1)
        t = np.sort(np.stack([src, dst, c], 1), 1)
        in_t = np.isin((t[:, 0] * B + t[:, 1]) * B + t[:, 2], self.triple_keys)
        in_p = np.isin(np.minimum(src, c) * B + np.maximum(src, c), self.pair_keys)
        return np.where((c == src) | in_t, 0, np.where(in_p, 1, 2))


def walks(graph, num_walks=40, walk_length=80, seed=0, max_trials=1024, nodes=None, count_trials=False):
    """(walks int32 [n * num_walks, walk_length], status int32 [4]) of matcha_amd.walk.hyper_walks.  ``count_trials``: also (proposals made
    at steps >= 2, proposals accepted there)."""
    T = graph if isinstance(graph, Tables) else Tables(graph)
    nodes = np.arange(1, T.N + 1, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
    W = len(nodes) * num_walks
    key = R.make_key(seed, STREAM_WALK)
    wid = np.arange(W, dtype=np.uint64)
    out = np.zeros((W, walk_length), dtype=np.int32)
    cur = nodes[np.arange(W) % len(nodes)].copy()
    prev = cur.copy()
    out[:, 0] = cur
    status = np.zeros(4, dtype=np.int32)
    made = taken = 0
    for s in range(1, walk_length):
        begin, count = T.ptr[cur], T.ptr[cur + 1] - T.ptr[cur]
        nxt = cur.copy()
        todo = np.flatnonzero(count > 0)
        for t in range(max_trials):
            if todo.size == 0:
                break
            ctr = np.uint64((s << 18) | (t << 2))
            c = T.nb[begin[todo] + cum_draw(T.cum, begin[todo], count[todo], rand_u64(key, wid[todo], ctr))]
            nxt[todo] = c
            if s == 1:
                todo = todo[:0]
                break
            thr = T.thr[T.classes(prev[todo], cur[todo], c)]
            ok = R.rand_u32(key, wid[todo], ctr | np.uint64(2)).astype(np.uint64) < thr
            made += todo.size
            taken += int(ok.sum())
            todo = todo[~ok]
        status[1] += todo.size
        prev, cur = cur, nxt
        out[:, s] = cur
    return (out, status, made, taken) if count_trials else (out, status)


# ---- skip-gram -----------------------------------------------------------------------------------------------------------------------
def _dot(a, b, dtype, order):
    if dtype == np.float64:
        return float(np.dot(a, b))
    prod = (a * b).astype(np.float32)
    if order == "seq":
        acc = np.float32(0)
        for x in prod:
            acc = np.float32(acc + x)
        return acc
    while prod.size > 1:                         # pairwise tree
        prod = (prod[0::2] + prod[1::2]).astype(np.float32)
    return prod[0]


def draws(W, Lw, g_base, noise_cum, window, negative, seed):
    """What the kernel draws for every position of a pass: (b int64 [W Lw] the reduced windows, ids int64 [W Lw, 2 window + 1, negative] the
    negatives of context slot jj = j - (i - window))."""
    key = R.make_key(seed, STREAM_SGNS)
    g = (np.uint64(g_base) + np.arange(W * Lw, dtype=np.uint64))
    b = window - (R.rand_u32(key, g, 0).astype(np.int64) % window)
    ids = np.zeros((W * Lw, 2 * window + 1, negative), dtype=np.int64)
    if negative:
        jj = np.arange(2 * window + 1, dtype=np.uint64)[None, :, None]
        k = np.arange(negative, dtype=np.uint64)[None, None, :]
        lo = np.broadcast_to(np.uint64(1) + np.uint64(2) * (jj * np.uint64(negative) + k), ids.shape)
        u = rand_u64(key, np.broadcast_to(g[:, None, None], ids.shape).ravel(), lo.ravel())
        cum = np.asarray(noise_cum).astype(np.uint64)[1:]
        ids = (1 + cum_draw(cum, np.zeros(u.size, dtype=np.int64), np.full(u.size, len(cum), dtype=np.int64), u)).reshape(ids.shape)
    return b, ids


@np.errstate(over="ignore")                             # exp(-f) of a dot product below -88 is +inf in float32, as expf's is: sigmoid 0
def sgns(walks_arr, syn0, syn1, noise_cum, window=10, negative=5, lr0=0.025, lr1=1e-4, epoch=0, epochs=1, seed=0, dtype=np.float64,
         order="seq", drawn=None, n_nodes=None, bad=None):
    """One pass over ``walks_arr`` [W, Lw] in sequence, on copies: returns (syn0, syn1) in ``dtype``.  ``drawn`` (a list) collects every
    negative id drawn.  (float64 takes a context's targets in one matrix product where its negatives are distinct: the same arithmetic,
    a target's update touches only its own row.)  ``n_nodes``: the kernel's rule for ids outside 1 .. n_nodes -- such a centre trains
    nothing, such a context is skipped, and ``bad`` (a list) collects the (w, i, j) at which one was met (j = i for a centre)."""
    walks_arr = np.asarray(walks_arr)
    W, Lw = walks_arr.shape
    s0, s1 = np.array(syn0, dtype=dtype), np.array(syn1, dtype=dtype)
    g_base, g_total = epoch * W * Lw, epochs * W * Lw
    b_all, neg_all = draws(W, Lw, g_base, noise_cum, window, negative, seed)
    one = dtype(1)
    for w in range(W):
        for i in range(Lw):
            center = int(walks_arr[w, i])
            if n_nodes is not None and not 1 <= center <= n_nodes:
                if bad is not None:
                    bad.append((w, i, i))
                continue
            g = g_base + w * Lw + i
            lr = dtype(np.float32(max(lr1, lr0 - (lr0 - lr1) * float(g) / float(g_total))))
            u = s1[center].copy()
            u0 = u.copy()
            b = int(b_all[w * Lw + i])
            for j in range(max(0, i - b), min(Lw - 1, i + b) + 1):
                if j == i:
                    continue
                ctx = int(walks_arr[w, j])
                if n_nodes is not None and not 1 <= ctx <= n_nodes:
                    if bad is not None:
                        bad.append((w, i, j))
                    continue
                v = s0[ctx].copy()
                f = _dot(v, u, dtype, order)
                gt = dtype((one - one / (one + np.exp(-dtype(f)))) * lr)
                neu = (gt * u).astype(dtype)
                u = (u + gt * v).astype(dtype)
                ids = neg_all[w * Lw + i, j - (i - window)]
                if drawn is not None:
                    drawn.extend(ids.tolist())
                ids = ids[ids != center]
                if dtype == np.float64 and len(np.unique(ids)) == len(ids):
                    t = s1[ids]
                    gts = (0.0 - 1.0 / (1.0 + np.exp(-(t @ v)))) * lr
                    neu = neu + gts @ t
                    s1[ids] = t + gts[:, None] * v[None, :]
                else:
                    for t_id in ids.tolist():
                        t = s1[t_id].copy()
                        f = _dot(v, t, dtype, order)
                        gt = dtype((dtype(0) - one / (one + np.exp(-dtype(f)))) * lr)
                        neu = (neu + gt * t).astype(dtype)
                        s1[t_id] = (s1[t_id] + gt * v).astype(dtype)
                s0[ctx] = (s0[ctx] + neu).astype(dtype)
            s1[center] = (s1[center] + (u - u0)).astype(dtype)
    return s0, s1


def sgns_loss(syn0, syn1, pairs, neg):
    """Mean skip-gram loss in float64 over an evaluation set: pairs int [n, 2] (context, centre), neg int [n, K] negatives of each."""
    s0, s1 = np.asarray(syn0, dtype=np.float64), np.asarray(syn1, dtype=np.float64)
    v = s0[pairs[:, 0]]
    pos = np.einsum("nd,nd->n", v, s1[pairs[:, 1]])
    ng = np.einsum("nd,nkd->nk", v, s1[neg])
    return float(np.mean(np.logaddexp(0, -pos) + np.logaddexp(0, ng).sum(1)))
