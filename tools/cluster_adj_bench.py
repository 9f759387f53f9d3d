"""Measure the contact matrices from clusters: pairs/s of the update kernel and the time of the finish.

    python tools/cluster_adj_bench.py [--shape a b c] [--repeat 5]

``a``: the hg38 1 Mb layout (N = 3 067), 2 000 000 clusters of 2 .. 25 nodes.  ``b``: the same plus 2 000 clusters of 1 000 nodes -- the skew
case: 2 000 clusters carry 4.6 times the pairs of the other two million.  ``c``: N = 30 344 (100 kb bins) with the clusters of ``a``, spread over
the larger range.  Clusters are synthetic (a random start and random positive gaps, so ids ascend).  ``kernel_seconds`` times
matcha_cluster_adj_update alone on device-resident inputs; ``update_seconds`` the whole ``ClusterAdj.update`` from host arrays (the host's prefix
sum, four host-to-device copies, the launch); ``finish_seconds`` the split finish.  Medians of ``--repeat`` runs after one warm-up, between
device synchronisations.  Prints one JSON line per shape.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matcha_amd import _lib, process as PC, synth  # noqa: E402

SHAPES = {"a": dict(n=3067, m=2000000, big=0), "b": dict(n=3067, m=2000000, big=2000), "c": dict(n=30344, m=2000000, big=0)}
BIG_SIZE, MAX_SMALL = 1000, 25


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def make_clusters(n, m, big, seed=7):
    """(ids int32, offsets int64) of m clusters of 2 .. 25 ascending ids in 1 .. n, then `big` clusters of 1 000 nodes, shuffled in."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, MAX_SMALL + 1, size=m)
    step = n // (MAX_SMALL + 1)
    pos = np.cumsum(rng.integers(1, step + 1, size=(m, MAX_SMALL), dtype=np.int32), axis=1, dtype=np.int32)
    keep = np.arange(MAX_SMALL)[None, :] < sizes[:, None]
    if not big:
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return np.ascontiguousarray(pos[keep], dtype=np.int32), offsets
    where = np.sort(rng.choice(m, size=big, replace=False))                   # the large clusters stand at random places of the list
    parts, lens, prev = [], [], 0
    for w in where:
        parts.append(pos[prev:w][keep[prev:w]])
        lens.append(sizes[prev:w])
        parts.append(np.sort(rng.choice(np.arange(1, n + 1, dtype=np.int32), size=BIG_SIZE, replace=False)))
        lens.append(np.asarray([BIG_SIZE]))
        prev = w
    parts.append(pos[prev:][keep[prev:]])
    lens.append(sizes[prev:])
    lens = np.concatenate(lens)
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def node2chrom(n):
    if n == 3067:
        return np.concatenate([[-1], synth.node2chrom(synth.LAYOUTS["hg38_1mb"])[1:]]).astype(np.int32)
    bounds = np.linspace(0, n, 24).astype(np.int64)                           # 23 blocks
    return np.concatenate([[-1], np.repeat(np.arange(23), np.diff(bounds))]).astype(np.int32)


def bench(name, repeat):
    shape = SHAPES[name]
    N = shape["n"]
    ids, offsets = make_clusters(N, shape["m"], shape["big"])
    lens = np.diff(offsets)
    pairs = int((lens * (lens - 1) // 2).sum())
    n2c = node2chrom(N)
    lib = _lib.load()
    dev = torch.device("cuda")
    # the kernel alone, on device-resident inputs
    pair_ptr = np.concatenate([[0], np.cumsum(lens * (lens - 1) // 2)]).astype(np.int64)
    q = PC.cluster_weights_q(lens, "one")
    d = [torch.from_numpy(a).to(dev) for a in (ids, offsets, q, pair_ptr)]
    acc = torch.zeros((N, N), dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        _lib.check(lib.matcha_cluster_adj_update(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), len(lens), N, _lib.ptr(acc),
                                                 _lib.ptr(status), st), "matcha_cluster_adj_update")
    t_kernel = timed(kernel, repeat)
    assert int(status[0]) == 0
    del acc
    # the public path
    ca = PC.ClusterAdj(N, n2c)
    t_update = timed(lambda: ca.update((ids, offsets), "one"), repeat)
    t_finish = timed(lambda: ca.finish(), repeat)
    intra, inter = ca.finish()
    total = float(intra.sum() + inter.sum())
    assert ca.status()[0] == 0 and total == 2.0 * pairs * (repeat + 1), (total, pairs)      # every pair, both triangles, once per update
    print(json.dumps(dict(what="cluster_adj", shape=name, nodes=N, clusters=int(len(lens)), ids=int(len(ids)), pairs=pairs,
                          largest_cluster=int(lens.max()), kernel_seconds=t_kernel, pairs_per_s=pairs / t_kernel, update_seconds=t_update,
                          finish_seconds=t_finish, finish_bytes=4 * N * N + 16 * N * N)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), nargs="*", default=["a", "b", "c"])
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    for name in a.shape:
        bench(name, a.repeat)


if __name__ == "__main__":
    main()
