"""Write tests/golden/cluster_adj_tiny.npz: the reference's own cluster -> contact-matrix projections on a small graph.

    python tools/make_cluster_adj_golden.py --reference <the reference's root directory>

Two functions of the reference run here, neither restated: ``edgelist2adj`` of ``Code/process.py`` and ``get_adjacency`` of
``History_version/Code/main_drop.py``.  Both modules run a whole script at import (and the first imports h5py), so the SOURCE of the one
function is cut out of each file with ``ast`` and executed with the globals it reads: ``temp_dir``, ``np``, ``os``, ``tqdm`` for the first
(it loads ``edge_list.npy`` / ``chrom_range.npy`` from ``temp_dir`` and saves ``edge_list_adj.npy`` there); ``num``, ``num_list``, ``np``,
``tqdm``, ``csr_matrix`` for the second.

The graph: 70 nodes in three chromosomes of 30, 25 and 15; clusters of 2, 3, 5 and 12 nodes, one of 40 nodes that spans all three
chromosomes, the pair (4, 33) alone in 7 clusters, node 70 in no cluster; integer weights 1 .. 9 for the weighted case.  Node ids in the file
are the project's 1-based ids (the History function gets them minus one).
"""
import argparse
import ast
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM = [30, 25, 15]
N_NODES = sum(NUM)


def function_source(path, name):
    with open(path) as f:
        text = f.read()
    for node in ast.parse(text).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return ast.get_source_segment(text, node)
    raise SystemExit("%s has no function %s" % (path, name))


def make_clusters():
    rng = np.random.default_rng(20240918)
    nodes = np.arange(1, N_NODES)                                             # node 70 stays out of every cluster
    clusters = []
    for size, count in ((2, 20), (3, 14), (5, 12), (12, 6)):
        for _ in range(count):
            clusters.append(sorted(rng.choice(nodes, size=size, replace=False).tolist()))
    big = np.concatenate([rng.choice(np.arange(1, 31), 17, replace=False), rng.choice(np.arange(31, 56), 14, replace=False),
                          rng.choice(np.arange(56, 70), 9, replace=False)])
    clusters.append(sorted(big.tolist()))                                     # 40 nodes over the three chromosomes
    clusters += [[4, 33]] * 7
    order = rng.permutation(len(clusters))
    clusters = [clusters[i] for i in order]
    weights = rng.integers(1, 10, size=len(clusters)).astype(np.float64)
    return clusters, weights


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="the reference's root (holds Code/process.py and History_version/Code/main_drop.py)")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "cluster_adj_tiny.npz"))
    a = ap.parse_args()
    from scipy.sparse import csr_matrix

    def tqdm(x, *args, **kw):
        return x

    clusters, weights = make_clusters()
    bounds = np.concatenate([[0], np.cumsum(NUM)])
    chrom_range = np.stack([bounds[:-1] + 1, bounds[1:] + 1], axis=1).astype(np.int64)

    # edgelist2adj: files in, file out
    with tempfile.TemporaryDirectory() as tmp:
        arr = np.empty(len(clusters), dtype=object)
        for i, c in enumerate(clusters):
            arr[i] = c
        np.save(os.path.join(tmp, "edge_list.npy"), arr, allow_pickle=True)
        np.save(os.path.join(tmp, "chrom_range.npy"), chrom_range)
        env = {"np": np, "os": os, "tqdm": tqdm, "temp_dir": tmp, "print": lambda *args, **kw: None}
        exec(function_source(os.path.join(a.reference, "Code", "process.py"), "edgelist2adj"), env)
        env["edgelist2adj"]()
        adj_one = np.load(os.path.join(tmp, "edge_list_adj.npy"))

    # get_adjacency: 0-based ids, num = nodes per type, num_list = their running totals
    env = {"np": np, "tqdm": tqdm, "csr_matrix": csr_matrix, "num": np.asarray(NUM), "num_list": list(np.cumsum(NUM))}
    exec(function_source(os.path.join(a.reference, "History_version", "Code", "main_drop.py"), "get_adjacency"), env)
    data = [np.asarray(c, dtype=np.int64) - 1 for c in clusters]
    adj_w = env["get_adjacency"](data, weights, False)
    adj_norm = env["get_adjacency"](data, weights, True)
    assert adj_one.shape == (N_NODES, N_NODES) and adj_one.dtype == np.float64
    assert adj_w.dtype == np.float32 and adj_norm.dtype == np.float32

    ids = np.concatenate([np.asarray(c, dtype=np.int32) for c in clusters])
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int64)
    node2chrom = np.concatenate([[-1], np.repeat(np.arange(len(NUM)), NUM)]).astype(np.int32)
    np.savez_compressed(a.out, ids=ids, offsets=offsets, weights=weights, n_nodes=np.int64(N_NODES), num=np.asarray(NUM, dtype=np.int64),
                        chrom_range=chrom_range, node2chrom=node2chrom, edgelist2adj=adj_one,
                        adjacency=np.asarray(adj_w.todense(), dtype=np.float32), adjacency_norm=np.asarray(adj_norm.todense(), dtype=np.float32))
    print("%s: %d clusters, %d ids, %d bytes" % (a.out, len(clusters), len(ids), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
