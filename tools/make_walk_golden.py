"""Write tests/golden/walk_tiny.npz: the reference's own transition probabilities of the hypergraph walk on a small graph.

    python tools/make_walk_golden.py --reference <the reference's History_version/Code directory>

The reference's random_walk_hyper.py is IMPORTED from that directory (nothing of it is restated here) and its two table builders,
``get_first_order_part`` and ``get_alias_n2n_2nd``, run in-process.  It was written for an older numpy and for an 80-process pool, so
three shims go in first: ``np.int``, ``np.array`` on ragged lists (an object array, as numpy < 1.24 gave), and the module globals that its
pool drivers set before they fork.  The probabilities are read back out of the alias tables it returns: outcome k of a table (J, q) over K
outcomes has mass (q[k] + sum over i with J[i] == k of (1 - q[i])) / K.

The graph: 16 nodes, hyperedges of sizes 2 .. 5; node 1 is a hub with more than 64 incidences, node 15 has exactly one incidence, node 16
is isolated; every second-order class (back / pair / far) occurs.  Node ids in the file are the project's 1-based ids.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, P, Q = 16, 2.0, 0.25


def make_edges():
    rng = np.random.default_rng(20240607)
    rows = set()
    while len(rows) < 22:                                  # the hub's edges: node 1 and 1 .. 4 of the nodes 2 .. 13
        k = int(rng.integers(2, 6))
        rows.add((1,) + tuple(sorted(rng.choice(np.arange(2, 14), size=k - 1, replace=False).tolist())))
    while len(rows) < 34:                                  # edges without the hub
        k = int(rng.integers(2, 6))
        rows.add(tuple(sorted(rng.choice(np.arange(2, 14), size=k, replace=False).tolist())))
    rows.add((3, 9, 14))
    rows.add((14, 15))                                     # node 15: one incidence
    rows = sorted(rows)
    out = np.zeros((len(rows), 5), dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out[rng.permutation(len(out))]                  # input order is not sorted order


def alias_probs(table):
    J, q = table
    q = np.minimum(np.asarray(q, dtype=np.float64), 1.0)
    K = len(q)
    mass = q.copy()
    np.add.at(mass, np.asarray(J, dtype=np.int64), 1.0 - q)
    return mass / K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="the directory that holds the reference's random_walk_hyper.py")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "walk_tiny.npz"))
    a = ap.parse_args()

    # shim 1 and 2: the numpy the reference was written for
    np.int = int
    plain_array = np.array

    def ragged_array(obj, *args, **kw):
        try:
            return plain_array(obj, *args, **kw)
        except ValueError:
            return plain_array(obj, *args, dtype=object, **kw)
    np.array = ragged_array
    sys.path.insert(0, os.path.abspath(a.reference))
    import random_walk_hyper as H

    edges = make_edges()
    hyperedges = [np.asarray(r[r != 0] - 1, dtype=np.int64) for r in edges]      # the reference's ids are 0-based (its toint)
    nodes = np.arange(N_NODES)
    G = H.HyperGraphRandomWalk(P, Q)
    G.build_graph(nodes, hyperedges)
    H.get_src_dst2e(G, np.arange(len(hyperedges)))
    # shim 3: the globals of get_first_order / parallel_get_second_order
    H.EV, H.VE, H.EV_over_delta, H.VE_over_delta = G.EV, G.VE, G.EV_over_delta, G.VE_over_delta
    H.node_nbr, H.node_degree, H.src_dst_2e, H.p, H.q = G.node_nbr, G.node_degree, G.src_dst_2e, G.p, G.q
    with_nbr = [v for v in nodes if len(G.node_nbr[v]) > 0]
    alias_1st, ff_1st = H.get_first_order_part(with_nbr)
    H.node2ff_1st = ff_1st

    first_ptr, first_nb, first_p = [0], [], []
    for v in nodes:
        if v in alias_1st:
            first_nb += [int(c) + 1 for c in G.node_nbr[v]]
            first_p += alias_probs(alias_1st[v]).tolist()
        first_ptr.append(len(first_nb))
    pair_src, pair_dst, second_ptr, second_p = [], [], [0], []
    for src in with_nbr:
        for dst in G.node_nbr[src]:
            pair_src.append(int(src) + 1)
            pair_dst.append(int(dst) + 1)
            second_p += alias_probs(H.get_alias_n2n_2nd(src, dst)).tolist()      # over nbr(dst), ascending
            second_ptr.append(len(second_p))
    np.array = plain_array
    np.savez(a.out, edges=edges, n_nodes=np.int64(N_NODES), p=np.float64(P), q=np.float64(Q),
             first_ptr=np.asarray(first_ptr, dtype=np.int64), first_nb=np.asarray(first_nb, dtype=np.int64),
             first_p=np.asarray(first_p, dtype=np.float64), pair_src=np.asarray(pair_src, dtype=np.int64),
             pair_dst=np.asarray(pair_dst, dtype=np.int64), second_ptr=np.asarray(second_ptr, dtype=np.int64),
             second_p=np.asarray(second_p, dtype=np.float64))
    print("%s: %d hyperedges, %d ordered pairs, %d second-order cells" % (a.out, len(edges), len(pair_src), len(second_p)))


if __name__ == "__main__":
    main()
