"""Measure the walk initialisation: walk steps/s, skip-gram pairs/s beside the derived atomic bound, the acceptance rate.

    python tools/walk_bench.py [--shape sprite|large] [--d 64] [--repeat 5] [--auroc]

``sprite``: 2 745 nodes, 340 000 random triples, 40 walks of 80 nodes per node (the shape of the reference's SPRITE run; the triples are
synthetic).  ``large``: 100 000 nodes, 2 000 000 hyperedges of 3 .. 5 nodes, 10 x 40.  Times are medians of ``--repeat`` runs after one warm-up,
between device synchronisations.  ``--auroc``: the validation AUROC after phase 1 of matcha_amd.train's table front end on synthetic data,
--table-init walk against random, same seeds.  Per shape also what one skip-gram pass learns (mean loss over evaluation pairs).
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matcha_amd import synth, walk as Wk  # noqa: E402

SHAPES = {"sprite": dict(n=2745, m=340000, ks=(3,), num_walks=40, walk_length=80),
          "large": dict(n=100000, m=2000000, ks=(3, 4, 5), num_walks=10, walk_length=40)}
ATOMIC_BYTES_PER_S = 1.3e12          # the chip-wide rate of row-shaped float atomic adds (the kernel guide's figure)


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


def make_graph(shape):
    edges = synth.make_edges_device(shape["n"], shape["m"], ks=shape["ks"], seed=5)
    edges = torch.unique(edges, dim=0)
    return Wk.HyperWalkGraph(edges, shape["n"]), edges


def bench(name, d, repeat, window=10, negative=5):
    shape = SHAPES[name]
    graph, edges = make_graph(shape)
    nw, lw = shape["num_walks"], shape["walk_length"]
    t_walk = timed(lambda: Wk.hyper_walks(graph, nw, lw, seed=1), repeat)
    walks, status = Wk.hyper_walks(graph, nw, lw, seed=1)
    steps = walks.shape[0] * (lw - 1)
    # acceptance per trial, from a capped run: with max_trials = 1 a step at s >= 2 is refused with probability 1 - acceptance
    _, st1 = Wk.hyper_walks(graph, nw, lw, seed=1, max_trials=1)
    later = walks.shape[0] * (lw - 2)
    print(json.dumps(dict(what="walk", shape=name, nodes=shape["n"], hyperedges=int(edges.shape[0]), incidences=int(graph.inc_nb.numel()),
                          walks=int(walks.shape[0]), walk_length=lw, seconds=t_walk, steps_per_s=steps / t_walk,
                          capped_steps=int(status[1]), acceptance_per_trial=1.0 - int(st1[1]) / max(1, later))))
    syn0, syn1 = Wk.sgns_init(shape["n"], d, 1)
    noise = Wk.noise_table(walks, shape["n"])
    t_sgns = timed(lambda: Wk.sgns_epoch(walks, syn0, syn1, noise, window, negative, seed=1), repeat)       # launches sized by sgns_epoch
    t_one = timed(lambda: Wk.sgns_epoch(walks, syn0, syn1, noise, window, negative, seed=1, chunk_walks=walks.shape[0]), repeat)
    # pairs of one pass: per position the contexts inside the walk at the mean reduced window (window + 1) / 2
    i = np.arange(lw)
    pairs = walks.shape[0] * float(np.mean([np.minimum(i, b).sum() + np.minimum(lw - 1 - i, b).sum() for b in range(1, window + 1)]))
    bytes_per_pair = 4.0 * d * (negative + 1) + 4.0 * d / max(1.0, pairs / (walks.shape[0] * lw))
    print(json.dumps(dict(what="sgns", shape=name, d=d, window=window, negative=negative, seconds=t_sgns, seconds_one_launch=t_one, pairs=pairs, pairs_per_s=pairs / t_sgns,
                          atomic_bytes_per_pair=bytes_per_pair, atomic_bound_pairs_per_s=ATOMIC_BYTES_PER_S / bytes_per_pair)))


def sgns_loss(syn0, syn1, pairs, neg):
    """Mean skip-gram loss in float64 over (context, centre) pairs with their negatives, on the device."""
    s0, s1 = syn0.double(), syn1.double()
    v = s0[pairs[:, 0]]
    pos = (v * s1[pairs[:, 1]]).sum(1)
    ng = torch.einsum("nd,nkd->nk", v, s1[neg])
    return float((torch.nn.functional.softplus(-pos) + torch.nn.functional.softplus(ng).sum(1)).mean())


def learning(name, d, window=10, negative=5):
    """What one pass learns at this shape: the mean loss over 20 000 evaluation pairs (adjacent walk positions, 5 uniform negatives), from
    the initial tables, after the default pass (launches sized by positions per node) and after the same pass as ONE launch."""
    shape = SHAPES[name]
    graph, _ = make_graph(shape)
    walks, _ = Wk.hyper_walks(graph, shape["num_walks"], shape["walk_length"], seed=1)
    noise = Wk.noise_table(walks, shape["n"])
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = torch.randint(0, walks.shape[0], (20000,), generator=g, device="cuda")
    cols = torch.randint(0, walks.shape[1] - 1, (20000,), generator=g, device="cuda")
    pairs = torch.stack([walks[rows, cols + 1], walks[rows, cols]], 1).long()
    neg = torch.randint(1, shape["n"] + 1, (20000, negative), generator=g, device="cuda")
    out = dict(what="sgns_loss", shape=name, d=d)
    syn0, syn1 = Wk.sgns_init(shape["n"], d, 1)
    out["initial"] = sgns_loss(syn0, syn1, pairs, neg)
    W, Lw = walks.shape
    out["walks_per_launch"] = min(1 << 20, -(-W // Wk.SGNS_MIN_LAUNCHES), max(1, Wk.SGNS_POSITIONS_PER_NODE * shape["n"] // Lw))
    Wk.sgns_epoch(walks, syn0, syn1, noise, window, negative, seed=1)
    out["default_pass"] = sgns_loss(syn0, syn1, pairs, neg)
    syn0, syn1 = Wk.sgns_init(shape["n"], d, 1)
    Wk.sgns_epoch(walks, syn0, syn1, noise, window, negative, seed=1, chunk_walks=-(-W // Wk.SGNS_MIN_LAUNCHES))
    out["64_launches"] = sgns_loss(syn0, syn1, pairs, neg)
    syn0, syn1 = Wk.sgns_init(shape["n"], d, 1)
    Wk.sgns_epoch(walks, syn0, syn1, noise, window, negative, seed=1, chunk_walks=W)
    out["one_launch"] = sgns_loss(syn0, syn1, pairs, neg)
    print(json.dumps(out))


def write_temp_dir(tmp, layout, k, m, d, seed=0):
    """A synthetic temp_dir and config as matcha_amd.train reads them (table front end: no adjacency needed)."""
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(seed)
    temp = os.path.join(tmp, "Temp")
    os.makedirs(temp)
    np.save(os.path.join(temp, "chrom_range.npy"), synth.chrom_range(num))
    n2c = synth.node2chrom(num)
    np.save(os.path.join(temp, "node2chrom.npy"), {int(i): int(n2c[i]) for i in range(1, N + 1)}, allow_pickle=True)
    np.save(os.path.join(temp, "all_%d_counter.npy" % k), synth.make_edges(rng, N, k, m))
    np.save(os.path.join(temp, "all_%d_freq_counter.npy" % k), synth.make_freq(rng, m))
    return {"temp_dir": temp, "min_distance": 0, "k-mer_size": [k], "quantile_cutoff_for_positive": 0.6, "quantile_cutoff_for_unlabel": 0.4,
            "embed_dim": d}


def auroc(d=64):
    """The validation lines of matcha_amd.train --front-end table on synthetic data, --table-init walk against random, same seeds: after
    phase 1 (alpha = 0: only the reconstruction term is trained, which the table front end does not have, so this line shows what the
    INITIAL table gives the untrained classifier) and after each of two short epochs of phase 2."""
    from matcha_amd import train as T
    for init in ("random", "walk"):
        with tempfile.TemporaryDirectory() as tmp:
            cfg = write_temp_dir(tmp, "c23", 3, 20000, d)
            np.random.seed(0)
            torch.manual_seed(0)
            logs = []
            T.run(cfg, front_end="table", epochs1=1, epochs2=2, batches_per_epoch=200, emb_path=None, log=logs.append, table_init=init)
            print(json.dumps(dict(what="auroc", table_init=init, validation=[l for l in logs if "Validation" in l])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), nargs="*", default=["sprite"])
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--auroc", action="store_true")
    a = ap.parse_args()
    for name in a.shape:
        bench(name, a.d, a.repeat)
        learning(name, a.d)
    if a.auroc:
        auroc(a.d)


if __name__ == "__main__":
    main()
