"""Initial bin embeddings for the table front end: hypergraph random walks + skip-gram with negative sampling.  

The reference's only use of ``Wrap_Embedding`` (History_version/Code/main_SPRITE.py:637-765, ``--feature walk``) does not start the table
from random normals: it samples biased second-order random walks over the hypergraph of the positive k-mers (random_walk_hyper.py), trains
gensim's skip-gram on them, standard-scales the vectors and loads them into the table behind a zero padding row.  This module is that
producer on the device:

* ``HyperWalkGraph`` -- the walk's tables: per node its incidence list with integer cumulative weights (the first-order distribution
  f(v, c) deg(c)^-1/2), the sets of all 2- and 3-subsets of the hyperedges (the second-order classes) and the classes' acceptance thresholds.
  Memory is one entry per incidence; the reference keeps one alias table per ordered pair of neighbours.
* ``hyper_walks`` -- matcha_hyper_walk (csrc/walk.hip): propose from the first-order distribution, accept with alpha / alpha_max.  Integer
  arithmetic throughout: tests/walk_ref.py reproduces every walk bit for bit.
* ``sgns_train`` -- matcha_sgns_epoch (csrc/sgns.hip): word2vec's skip-gram, one wavefront per corpus position, float atomics into the two
  tables.  NOT bitwise reproducible from run to run (the atomics' arrival order); frequent-word subsampling is left out.
* ``standard_scale``, ``walk_embeddings`` -- sklearn's StandardScaler and the whole chain, ``[N + 1, d]`` with a zero row 0.

Node ids are the project's 1-based ids (the reference subtracts 1): table row = node id, row 0 = padding.

CLI:  python -m matcha_amd.walk --config ./config.JSON -o wv.npy [--save-walks walks.txt]
writes the reference's two files: the unscaled vectors ``[N, d]`` (its ``<name>_wv_<d>_hyper.npy``) and, on request, the walks with
0-based ids as its ``np.savetxt(path, walks, fmt="%d", delimiter=" ")`` writes them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .sampler import HyperedgeSet

MAX_WIDTH = _lib.MAX_L              # the triple set grows as C(k, 3)
WEIGHT_BITS = 40                    # an incidence's weight is rint(2^40 deg(c)^-1/2 / |e|), at least 1
MAX_INCIDENCES = 1 << 24            # per node: the node's total stays below 2^63
STREAM_WALK, STREAM_SGNS = 19, 20   # kStreamWalk, kStreamSgns of csrc/common.hpp
CLASS_BACK, CLASS_PAIR, CLASS_FAR = 0, 1, 2
ALWAYS = 1 << 32                    # the threshold of the class that holds alpha_max
SGNS_MIN_LAUNCHES = 64              # a skip-gram pass is at least this many launches (sgns_epoch) ...
SGNS_POSITIONS_PER_NODE = 4         # ... and a launch holds at most this many corpus positions per node


def _subsets(edges: torch.Tensor, r: int) -> torch.Tensor:
    """The unique r-subsets of all rows of ``edges`` (zero-padded ascending), int64 [n, r], sorted lexicographically."""
    L = edges.shape[1]
    if L < r or edges.shape[0] == 0:
        return edges.new_zeros((0, r))
    comb = torch.combinations(torch.arange(L, device=edges.device), r)
    rows = edges[:, comb].reshape(-1, r)
    rows = rows[(rows != 0).all(1)]
    return torch.unique(rows, dim=0) if rows.shape[0] else rows


def class_thresholds(p: float, q: float):
    """[T_back, T_pair, T_far] for alpha = 1/p, 1, 1/q: floor(2^32 alpha / alpha_max), at most 2^32 - 1; a class that holds alpha_max
    accepts always (2^32: every 32-bit draw is below it)."""
    if not (p > 0 and q > 0 and math.isfinite(p) and math.isfinite(q)):
        raise ValueError(f"p={p} q={q}: both must be positive")
    alpha = [1.0 / p, 1.0, 1.0 / q]
    top = max(alpha)
    return [ALWAYS if a == top else min(ALWAYS - 1, int(math.floor(ALWAYS * (a / top)))) for a in alpha]


class HyperWalkGraph:
    """The tables of the hypergraph walk over ``edges`` int64 [M, L <= 8] (zero-padded ascending rows, sizes mixed), nodes 1 .. n_nodes.
    Built with torch ops on the device of ``edges``; on a cuda device the two subset sets are ``HyperedgeSet``s, on the CPU they stay the
    sorted tables ``pairs`` / ``triples`` (tests/walk_ref.py walks those).

    inc_ptr int64 [N + 2], inc_nb int32 [I], inc_cum int64 [I] (read as uint64): node v's incidences are inc_ptr[v] .. inc_ptr[v + 1], one
    per (hyperedge e of v in input order, other node c of e); inc_cum is the inclusive prefix inside the node of
    max(1, rint(2^40 deg(c)^-1/2 / |e|)).  Summed over the incidences of one neighbour that is f(v, c) deg(c)^-1/2 -- no de-duplication."""

    def __init__(self, edges, n_nodes: int, p: float = 2.0, q: float = 0.25):
        edges = torch.as_tensor(edges)
        if edges.dim() != 2:
            raise ValueError("HyperWalkGraph: edges must be [M, L]")
        M, L = int(edges.shape[0]), int(edges.shape[1])
        if L > MAX_WIDTH:
            raise ValueError(f"HyperWalkGraph: rows of {L} columns (at most {MAX_WIDTH}: the triple set grows as C(k, 3))")
        edges = edges.to(torch.long).contiguous()
        dev = edges.device
        N = int(n_nodes)
        if N < 1 or N >= (1 << 21):
            raise ValueError(f"HyperWalkGraph: n_nodes={N} outside 1 .. 2^21 - 1")
        nz = edges != 0
        k = nz.sum(1)
        if M:
            if int(edges.min()) < 0 or int(edges.max()) > N:
                raise ValueError(f"HyperWalkGraph: a node id outside 0 .. {N}")
            cols = torch.arange(L, device=dev)
            if not bool((nz == (cols[None, :] < k[:, None])).all()):
                raise ValueError("HyperWalkGraph: rows must be zero-padded behind their nodes")
            if L > 1 and not bool(((edges[:, 1:] > edges[:, :-1]) | ~nz[:, 1:]).all()):
                raise ValueError("HyperWalkGraph: rows must be strictly ascending")
        self.n_nodes, self.p, self.q, self.device = N, float(p), float(q), dev
        self.thresholds = class_thresholds(p, q)
        deg = torch.bincount(edges.reshape(-1), minlength=N + 1)
        deg[0] = 0
        self.deg = deg
        # one incidence per (e, i, j != i) with both slots used; nonzero() lists them in (e, i, j) order and the stable sort by the node
        # keeps that order inside a node
        mask = nz[:, :, None] & nz[:, None, :] & ~torch.eye(L, dtype=torch.bool, device=dev)[None]
        e_idx, i_idx, j_idx = mask.nonzero(as_tuple=True)
        v, c = edges[e_idx, i_idx], edges[e_idx, j_idx]
        order = torch.sort(v, stable=True).indices
        v, c, e_idx = v[order], c[order], e_idx[order]
        counts = torch.bincount(v, minlength=N + 1)
        if v.numel() and int(counts.max()) >= MAX_INCIDENCES:
            raise ValueError(f"HyperWalkGraph: a node with {int(counts.max())} incidences (fewer than 2^24 keep its total below 2^63)")
        ptr = torch.zeros(N + 2, dtype=torch.long, device=dev)
        ptr[1:] = torch.cumsum(counts, 0)
        # sqrt, the product with a small integer and the division are correctly rounded in float64 on the host and on the device
        w = torch.round(float(1 << WEIGHT_BITS) / (torch.sqrt(deg[c].double()) * k[e_idx].double())).clamp_(min=1.0).to(torch.long)
        # prefix inside the node = global prefix - the global prefix in front of the node, taken separately over the weights' high and low
        # 20 bits: a part is below 2^20, so its global prefix stays below 2^63 for any graph that fits in memory -- nothing wraps
        self.inc_ptr, self.inc_nb = ptr, c.to(torch.int32).contiguous()
        if v.numel():
            parts = []
            for part in (w >> 20, w & ((1 << 20) - 1)):
                tot = torch.cumsum(part, 0)
                parts.append(tot - (tot - part)[ptr[v]])
            self.inc_cum = ((parts[0] << 20) + parts[1]).contiguous()
        else:
            self.inc_cum = w
        self.pairs, self.triples = _subsets(edges, 2), _subsets(edges, 3)
        self.pair_set = HyperedgeSet(self.pairs) if dev.type == "cuda" else None
        self.triple_set = HyperedgeSet(self.triples) if dev.type == "cuda" else None
        self._keys = None

    # ---- the distribution the integers imply (host arithmetic; tests/test_cpu_walk.py holds it against the reference's alias tables) ----
    def _member_keys(self):
        if self._keys is None:
            B = self.n_nodes + 1
            pr, tr = self.pairs.cpu().numpy(), self.triples.cpu().numpy()
            self._keys = (np.sort(pr[:, 0] * B + pr[:, 1]), np.sort((tr[:, 0] * B + tr[:, 1]) * B + tr[:, 2]))
        return self._keys

    def classes(self, src: int, dst: int, cand) -> np.ndarray:
        """The second-order class (CLASS_BACK / CLASS_PAIR / CLASS_FAR) of every candidate next node after the step src -> dst."""
        cand = np.asarray(cand, dtype=np.int64)
        B = self.n_nodes + 1
        pk, tk = self._member_keys()
        t = np.sort(np.stack([np.full_like(cand, src), np.full_like(cand, dst), cand], 1), 1)
        in_t = np.isin((t[:, 0] * B + t[:, 1]) * B + t[:, 2], tk)
        in_p = np.isin(np.minimum(cand, src) * B + np.maximum(cand, src), pk)
        return np.where((cand == src) | in_t, CLASS_BACK, np.where(in_p, CLASS_PAIR, CLASS_FAR))

    def transition(self, src, dst: int):
        """(neighbours int64 [n] ascending, probabilities float64 [n]) of the step out of ``dst`` after ``src`` (None or 0: the first
        step), as the tables' integers give them: per neighbour the sum of weight x threshold over its incidences, normalised."""
        b, e = int(self.inc_ptr[dst]), int(self.inc_ptr[dst + 1])
        nb = self.inc_nb[b:e].cpu().numpy().astype(np.int64)
        cum = self.inc_cum[b:e].cpu().numpy().astype(np.uint64)
        w = np.diff(cum, prepend=np.uint64(0)).astype(np.float64)
        if src:
            w = w * np.asarray(self.thresholds, dtype=np.float64)[self.classes(int(src), int(dst), nb)]
        ids, inv = np.unique(nb, return_inverse=True)
        mass = np.bincount(inv, weights=w, minlength=len(ids))
        return ids, mass / mass.sum() if len(ids) else mass


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def hyper_walks(graph: HyperWalkGraph, num_walks: int = 40, walk_length: int = 80, seed: int = 0, max_trials: int = 1024, nodes=None,
                chunk_walks: int = 1 << 20):
    """(walks int32 [n * num_walks, walk_length], status int32 [4]) on the graph's device: walk w starts at nodes[w % n] (``nodes``: default
    every node 1 .. N), so the corpus interleaves the nodes.  status[1] counts the steps whose ``max_trials`` proposals were all refused
    (the last one stands).  The walks of a seed do not depend on ``chunk_walks``, the walks per launch."""
    lib = _lib.load()
    if graph.pair_set is None:
        raise _lib.MatchaHipError("hyper_walks needs a graph on a cuda device (no CPU fallback)")
    dev = graph.device
    nodes = torch.arange(1, graph.n_nodes + 1, dtype=torch.int32, device=dev) if nodes is None else \
        torch.as_tensor(nodes).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    n = int(nodes.numel())
    if n < 1 or num_walks < 1:
        raise ValueError(f"hyper_walks: {n} start nodes x {num_walks} walks")
    W = n * int(num_walks)
    walks = torch.empty(W, int(walk_length), dtype=torch.int32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    seed_t = torch.full((1,), int(seed), dtype=torch.int64, device=dev)
    thr = (C.c_int64 * 3)(*graph.thresholds)
    ps, ts = graph.pair_set, graph.triple_set
    for w0 in range(0, W, max(1, int(chunk_walks))):
        w1 = min(W, w0 + max(1, int(chunk_walks)))
        _lib.check(lib.matcha_hyper_walk(_lib.ptr(graph.inc_ptr), _lib.ptr(graph.inc_nb), _lib.ptr(graph.inc_cum), graph.n_nodes,
                                         _lib.ptr(ps.table), _lib.ptr(ps.edges), ps.n, ps.L, _lib.ptr(ts.table), _lib.ptr(ts.edges), ts.n, ts.L,
                                         thr, _lib.ptr(nodes), n, w0, w1, int(walk_length), int(max_trials), _lib.ptr(seed_t),
                                         _lib.ptr(walks[w0:w1]), _lib.ptr(status), _stream(walks)), "matcha_hyper_walk")
    return walks, status


# ---- skip-gram -----------------------------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _lowbias32(x: torch.Tensor) -> torch.Tensor:
    """oracle/rng.py's mixer on int64 tensors that hold 32-bit values."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _rng_key(seed: int, stream: int) -> int:
    one = lambda v: int(_lowbias32(torch.tensor([v & _M32], dtype=torch.long))[0])
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k = one(stream + 0x9E3779B9)
    k = one((seed >> 32) ^ k)
    return one((seed & _M32) ^ k)


def sgns_init(n_nodes: int, d: int, seed: int, device="cuda"):
    """(syn0, syn1) float32 [N + 1, d]: syn0[r, c] = ((rand(stream 20 of seed + 2^32, r, c) >> 8) 2^-24 - 0.5) / d -- word2vec's uniform
    +-0.5 / d, exact in float32 -- with a zero padding row 0; syn1 = 0."""
    key = _rng_key(int(seed) + (1 << 32), STREAM_SGNS)          # (its own seed: the training pass draws from stream 20 of `seed`)
    r = torch.arange(n_nodes + 1, dtype=torch.long, device=device)[:, None]
    c = torch.arange(d, dtype=torch.long, device=device)[None, :]
    u = _lowbias32(c ^ _lowbias32(r ^ key))
    syn0 = ((u >> 8).to(torch.float32) * (1.0 / 16777216.0) - 0.5) / float(d)
    syn0[0] = 0
    return syn0.contiguous(), torch.zeros_like(syn0)


def noise_table(walks: torch.Tensor, n_nodes: int) -> torch.Tensor:
    """int64 [N + 1] (read as uint64): the inclusive prefix over the ids of rint(2^32 count^0.75 / sum), entry 0 = 0 -- word2vec's unigram
    table as an integer cumulative table, drawn by inverse CDF like a walk's proposal."""
    cnt = torch.bincount(walks.reshape(-1).to(torch.long).clamp(0, n_nodes), minlength=n_nodes + 1).double()
    cnt[0] = 0
    pw = cnt.pow(0.75)
    return torch.cumsum(torch.round(pw * (float(1 << 32) / float(pw.sum()))).to(torch.long), 0).contiguous()


def sgns_epoch(walks: torch.Tensor, syn0: torch.Tensor, syn1: torch.Tensor, noise_cum: torch.Tensor, window: int = 10, negative: int = 5,
               lr0: float = 0.025, lr1: float = 1e-4, epoch: int = 0, epochs: int = 1, seed: int = 0, chunk_walks=None):
    """One pass of matcha_sgns_epoch over ``walks`` int32 [W, Lw], updating syn0 / syn1 in place; returns the status word int32 [4]
    (status[0] & 1: an id outside 1 .. N was met and skipped).  Float atomics: not bitwise reproducible from run to run.

    The positions of one launch all read the tables as they stand and add into them; launches follow each other on the stream.  word2vec
    keeps a few dozen positions in flight (its threads); a whole small corpus in ONE launch is a single large-batch step instead of
    stochastic descent (from syn1 = 0 it moves syn1 alone).  What matters is how many positions meet in one row at once, so a launch takes
    ``chunk_walks`` walks with, by default, at most ``SGNS_POSITIONS_PER_NODE`` = 4 positions per node (the regime measured: 3 per node,
    DESIGN.md 7.17), at most 1/``SGNS_MIN_LAUNCHES`` of the pass and at most 2^20 walks."""
    lib = _lib.load()
    if not (walks.is_cuda and syn0.is_cuda and syn1.is_cuda):
        raise _lib.MatchaHipError("sgns_epoch needs cuda tensors (no CPU fallback)")
    assert walks.dtype == torch.int32 and walks.is_contiguous() and syn0.dtype == syn1.dtype == torch.float32
    assert syn0.is_contiguous() and syn1.is_contiguous() and syn0.shape == syn1.shape and noise_cum.numel() == syn0.shape[0]
    W, Lw = int(walks.shape[0]), int(walks.shape[1])
    N, d = int(syn0.shape[0]) - 1, int(syn0.shape[1])
    status = torch.zeros(4, dtype=torch.int32, device=walks.device)
    seed_t = torch.full((1,), int(seed), dtype=torch.int64, device=walks.device)
    chunk = min(1 << 20, -(-W // SGNS_MIN_LAUNCHES), max(1, SGNS_POSITIONS_PER_NODE * N // Lw)) if chunk_walks is None else int(chunk_walks)
    for w0 in range(0, W, max(1, chunk)):
        w1 = min(W, w0 + max(1, chunk))
        _lib.check(lib.matcha_sgns_epoch(_lib.ptr(walks), W, Lw, w0, w1, N, d, _lib.ptr(syn0), _lib.ptr(syn1), _lib.ptr(noise_cum),
                                         int(window), int(negative), float(lr0), float(lr1), int(epoch) * W * Lw, int(epochs) * W * Lw,
                                         _lib.ptr(seed_t), _lib.ptr(status), _stream(walks)), "matcha_sgns_epoch")
    return status


def sgns_train(walks: torch.Tensor, n_nodes: int, d: int, window: int = 10, negative: int = 5, lr0: float = 0.025, lr1: float = 1e-4,
               epochs: int = 1, seed: int = 0) -> torch.Tensor:
    """word2vec's skip-gram with negative sampling over ``walks`` (int32 [W, Lw], ids 1 .. N): syn0 float32 [N + 1, d], row 0 zero.
    The learning rate falls linearly from lr0 to lr1 over the epochs' positions.  Not bitwise reproducible from run to run."""
    if d not in (64, 128, 256):
        raise ValueError(f"sgns_train: d={d} (64, 128 or 256)")
    walks = walks.to(torch.int32).contiguous()
    syn0, syn1 = sgns_init(n_nodes, d, seed, walks.device)
    noise = noise_table(walks, n_nodes)
    bad = 0
    for ep in range(int(epochs)):
        st = sgns_epoch(walks, syn0, syn1, noise, window, negative, lr0, lr1, ep, epochs, seed)
        bad |= int(st[0])
    if bad & _lib.STATUS_BAD_ID:
        raise IndexError(f"sgns_train: a walk holds an id outside 1 .. {n_nodes}")
    return syn0


def standard_scale(A: torch.Tensor) -> torch.Tensor:
    """sklearn's StandardScaler().fit_transform: per column (x - mean) / population std, a constant column divided by 1."""
    A64 = A.double()
    mean = A64.mean(0, keepdim=True)
    std = (A64 - mean).pow(2).mean(0, keepdim=True).sqrt()
    std = torch.where(std < 10 * torch.finfo(torch.float64).eps, torch.ones_like(std), std)
    return ((A64 - mean) / std).to(A.dtype)


def walk_embeddings(edges, n_nodes: int, d: int, p: float = 2.0, q: float = 0.25, num_walks: int = 40, walk_length: int = 80,
                    window: int = 10, negative: int = 5, lr0: float = 0.025, lr1: float = 1e-4, epochs: int = 1, seed: int = 0,
                    max_trials: int = 1024, return_parts: bool = False):
    """The reference's table initialisation (main_SPRITE.py:637-765): walks over the hypergraph of ``edges`` (a cuda tensor), skip-gram,
    StandardScaler over the N node rows, a zero row 0: float32 [N + 1, d].  ``return_parts``: also (walks, unscaled syn0)."""
    graph = HyperWalkGraph(edges, n_nodes, p, q)
    walks, status = hyper_walks(graph, num_walks, walk_length, seed, max_trials)
    if int(status[0]) & _lib.STATUS_BAD_ID:
        raise IndexError("walk_embeddings: a start node outside the graph")
    syn0 = sgns_train(walks, n_nodes, d, window, negative, lr0, lr1, epochs, seed)
    table = torch.cat([torch.zeros_like(syn0[:1]), standard_scale(syn0[1:])]).contiguous()
    return (table, walks, syn0) if return_parts else table


def run(config: dict, out: str, save_walks=None, d=None, device: str = "cuda", log=print, **kw):
    """The CLI's body: the positives of temp_dir as matcha_amd.train loads them -> ``out`` (unscaled vectors float32 [N, d], the reference's
    <name>_wv_<d>_hyper.npy) and optionally the walk file (0-based ids, "%d" separated by blanks)."""
    from .train import load_kmers
    temp_dir = config["temp_dir"]
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy")).astype(np.int64)
    N = int(sum(int(v[1] - v[0]) for v in chrom_range))
    d = int(d or config["embed_dim"])
    data, _ = load_kmers(temp_dir, [int(v) for v in config["k-mer_size"]], float(config["quantile_cutoff_for_positive"]))
    edges = torch.from_numpy(np.ascontiguousarray(data).astype(np.int64)).to(device)
    table, walks, syn0 = walk_embeddings(edges, N, d, return_parts=True, **kw)
    np.save(out, syn0[1:].cpu().numpy())
    if save_walks:
        np.savetxt(save_walks, walks.cpu().numpy().astype(np.int64) - 1, fmt="%d", delimiter=" ")
    log("%d walks of %d nodes over %d hyperedges -> %s" % (walks.shape[0], walks.shape[1], edges.shape[0], out))
    return table


def main(argv=None):
    from . import utils as U
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="The skip-gram pass adds into its tables with float atomics: two runs of one seed agree in "
                                        "distribution, not bit for bit.")
    ap.add_argument("--config", default="./config.JSON")
    ap.add_argument("-o", "--out", required=True, help="the unscaled vectors, float32 [N, d] (.npy)")
    ap.add_argument("--save-walks", default=None, help="also write the walks, 0-based ids, one walk per line")
    ap.add_argument("-d", "--dimensions", type=int, default=None, help="64, 128 or 256 (default: the config's embed_dim)")
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--num-walks", type=int, default=40)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--p", type=float, default=2.0)
    ap.add_argument("--q", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    run(U.get_config(a.config), a.out, a.save_walks, a.dimensions, p=a.p, q=a.q, num_walks=a.num_walks, walk_length=a.walk_length,
        window=a.window, seed=a.seed)


if __name__ == "__main__":
    main()
