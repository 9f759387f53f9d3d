"""Outlier identification: which locus of a hyperedge does not belong?  

The benchmark Hyper-SAGNN was published with (the reference's History_version/Code/utils.py:184-233): plant ONE foreign bin of the same
chromosome in a positive (``generate_outlier_part``), ask the model for the positions it supports least (``model(inputs, get_outlier=k)``)
and count how often the planted bin is among them (``check_outlier``: "outlier top k hitting").  It needs no held-out labels.

* ``OutlierPlanter`` -- the plant on the device (matcha_outlier_plant, csrc/sampler.hip): per copy of a positive one position, a bin of that
  locus's chromosome drawn until the row is duplicate-free, has all adjacent gaps > min_dis, is no known hyperedge and -- with a pair set,
  the reference's ``dict_pair`` rule -- no known pair goes through the planted bin.
* ``Classifier.locus_scores(x, lowest=top)`` -- the per-locus scores of one forward and the ``top`` least supported slots.
* ``outlier_hits`` -- per hyperedge size the rows whose planted locus stands at rank r of that order; exact integer counts on the device.
* ``outlier_benchmark`` -- the three in chunks; per size and overall the rows, the cumulative hits and the chance level r / s.

CLI:  python -m matcha_amd.outlier --config ./config.JSON --model model2load --sizes 3 4 5 --top 3
(the positives and the known set from temp_dir's k-mers as matcha_amd.finetune loads them, the pair set from the size-2 k-mers when
temp_dir has them); prints the reference's "outlier top r hitting" lines per size, with chance beside them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from .sampler import HyperedgeSet, _check_width

CHUNK_ROWS = 65536
MIN_SIZE, MAX_SIZE = 2, _lib.MAX_LONG_L


class OutlierPlanter:
    """``draws`` copies of every positive with one locus replaced by a foreign bin of the same chromosome (matcha_outlier_plant; the rule
    is stated in include/matcha_hip.h and restated in tests/outlier_ref.py).  Shaped like ``NegativeSampler``: ``hset`` the known
    hyperedges (``HyperedgeSet.empty`` switches that refusal off), ``pair_set`` an optional ``HyperedgeSet`` of known pairs, ``node2chrom``
    int32 [N + 1], ``chrom_range`` int32 [C, 2].  The seed does not advance: row n of a seed is one fixed row, whichever call asks for it."""

    def __init__(self, hset: HyperedgeSet, node2chrom: np.ndarray, chrom_range: np.ndarray, pair_set: Optional[HyperedgeSet] = None,
                 min_dis: int = 0, seed: int = 0):
        dev = hset.edges.device
        self.hset, self.pair_set, self.min_dis = hset, pair_set, int(min_dis)
        if pair_set is not None and pair_set.n > 0 and pair_set.L < 2:
            raise ValueError("OutlierPlanter: the pair set holds rows of two nodes (its width is %d)" % pair_set.L)
        self.node2chrom = torch.as_tensor(np.asarray(node2chrom, dtype=np.int32), device=dev)
        self.chrom_range = torch.as_tensor(np.asarray(chrom_range, dtype=np.int32), device=dev).contiguous()
        self.seed = torch.full((1,), int(seed), dtype=torch.int64, device=dev)
        self.n_nodes = int(self.node2chrom.numel()) - 1
        self.n_chrom = int(self.chrom_range.shape[0])
        # device status word (include/matcha_hip.h): [0] bit 1 = a locus outside [1, N] or without a chromosome was met (no plant),
        # [1] = rows whose 256 trials were exhausted (returned equal to their positive, planted = -1)
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)

    def plant(self, pos: torch.Tensor, draws: int = 1, cycle: bool = False, n0: int = 0):
        """pos int64 [P, L] zero-padded ascending -> (rows int64 [P*draws, L], planted int32 [P*draws]): copies of positive j at rows
        draws*j ..., ``planted`` the index of the foreign locus in its row, -1 where none could be planted (the row is then its positive).
        ``cycle``: copy i replaces position i % k instead of a drawn one.  ``n0``: the global index of the first
        row -- a caller that cuts its positives into chunks passes draws * (positives in front of the chunk) and gets the rows of one call."""
        lib = _lib.load()
        pos = torch.as_tensor(pos).to(device=self.seed.device, dtype=torch.long).contiguous()
        P, L = pos.shape
        _check_width(int(L), "OutlierPlanter")
        rows = torch.empty(P * draws, L, dtype=torch.long, device=pos.device)
        planted = torch.empty(P * draws, dtype=torch.int32, device=pos.device)
        ps = self.pair_set if self.pair_set is not None and self.pair_set.n > 0 else None
        st = C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream)
        _lib.check(lib.matcha_outlier_plant(_lib.ptr(self.hset.table), _lib.ptr(self.hset.edges), self.hset.n, self.hset.L,
                                            _lib.ptr(ps.table) if ps else None, _lib.ptr(ps.edges) if ps else None, ps.n if ps else 0,
                                            ps.L if ps else 0, _lib.ptr(pos), P, L, int(draws), 1 if cycle else 0, self.min_dis,
                                            _lib.ptr(self.node2chrom), self.n_nodes, _lib.ptr(self.chrom_range), self.n_chrom,
                                            _lib.ptr(self.seed), int(n0), _lib.ptr(rows), _lib.ptr(planted), _lib.ptr(self.status), st),
                   "matcha_outlier_plant")
        return rows, planted

    def check_status(self) -> int:
        """Synchronising read of the status word: raises KeyError if a locus without a chromosome reached the planter; returns the number
        of rows whose 256 trials were exhausted since the last call."""
        st = self.status.tolist()
        self.status.zero_()
        _lib.raise_on_status(st, "OutlierPlanter")
        return int(st[1])


def outlier_hits(order: torch.Tensor, planted: torch.Tensor, sizes: torch.Tensor, top: int):
    """(rows int64 [33], hits int64 [33, top]) indexed by hyperedge size: ``rows[s]`` = the rows of size s (2 .. 32) with a planted locus
    (``planted`` >= 0), ``hits[s, r]`` = those of them with ``order[:, r] == planted`` -- the planted locus is the model's (r + 1)-th least
    supported one.  ``order`` int64 [n, m] (``locus_scores``'s; -1 behind a row's loci never matches), ranks r >= m count nothing.
    Integer ops on the tensors' device: exact, no synchronisation."""
    top = int(top)
    planted = planted.to(torch.long).view(-1)
    sizes = sizes.to(device=planted.device, dtype=torch.long).view(-1)
    order = order.to(device=planted.device, dtype=torch.long).view(planted.numel(), -1)
    valid = (planted >= 0) & (sizes >= MIN_SIZE) & (sizes <= MAX_SIZE)
    key = torch.where(valid, sizes, torch.zeros_like(sizes))            # invalid rows count into slot 0, cleared below
    rows = torch.zeros(MAX_SIZE + 1, dtype=torch.long, device=planted.device).index_add_(0, key, valid.to(torch.long))
    hits = torch.zeros(MAX_SIZE + 1, top, dtype=torch.long, device=planted.device)
    m = min(top, order.shape[1])
    if m > 0:
        hit = (order[:, :m] == planted.unsqueeze(1)) & valid.unsqueeze(1)
        hits[:, :m].index_add_(0, key, hit.to(torch.long))
    rows[0] = 0
    hits[0] = 0
    return rows, hits


def outlier_benchmark(model, positives, planter: OutlierPlanter, top: int = 3, draws: int = 1, cycle: bool = False,
                      chunk_rows: int = CHUNK_ROWS, keep: bool = False):
    """The planted-outlier benchmark on ``positives`` (int64 [M, W] zero-padded ascending, sizes 2 .. 32): per chunk of ``chunk_rows``
    positives plant (``n0`` = draws * positives in front, so the planted rows do not depend on ``chunk_rows``), score with
    ``model.locus_scores(rows, lowest=top)`` at the chunk's OWN width -- its longest row; a score depends on the width as a logit does --
    and count with ``outlier_hits``.  Returns

      {"top": top, "sizes": {s: entry}, "overall": entry},  entry = {"rows": n, "hit": [hit@1 .. hit@top], "chance": [1/s .. top/s]}

    ``hit`` cumulative COUNTS (the planted locus is among the r least supported), ``chance`` what a random order gives (min(r, s) / s;
    overall: its mean over the rows); sizes without a planted row are left out.  ``keep``: also "planted_rows", "planted", "order"
    (device tensors, rows padded to the widest chunk).  One host read at the end."""
    top = int(top)
    if top < 1 or top > MAX_SIZE:
        raise ValueError(f"top={top} outside 1 .. {MAX_SIZE}")
    dev = planter.seed.device
    pos = torch.as_tensor(positives).to(device=dev, dtype=torch.long)
    _check_width(int(pos.shape[1]), "outlier_benchmark")
    rows_t = torch.zeros(MAX_SIZE + 1, dtype=torch.long, device=dev)
    hits_t = torch.zeros(MAX_SIZE + 1, top, dtype=torch.long, device=dev)
    kept = []
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), model.deferred_id_check():
            for j in range(0, pos.shape[0], chunk_rows):
                chunk = pos[j:j + chunk_rows]
                width = max(MIN_SIZE, int((chunk != 0).sum(1).max()))
                rows, planted = planter.plant(chunk[:, :width].contiguous(), draws=draws, cycle=cycle, n0=j * draws)
                order = model.locus_scores(rows, lowest=top).order
                r, h = outlier_hits(order, planted, (rows != 0).sum(1), top)
                rows_t += r
                hits_t += h
                if keep:
                    kept.append((rows, planted, order))
    finally:
        model.train(was)
    n = rows_t.tolist()
    cum = hits_t.cumsum(1).tolist()
    out = {"top": top, "sizes": {}}
    for s in range(MIN_SIZE, MAX_SIZE + 1):
        if n[s]:
            out["sizes"][s] = {"rows": n[s], "hit": cum[s], "chance": [min(r, s) / s for r in range(1, top + 1)]}
    total = sum(n)
    out["overall"] = {"rows": total, "hit": [sum(cum[s][r] for s in range(MAX_SIZE + 1)) for r in range(top)],
                      "chance": [sum(n[s] * min(r, s) / s for s in range(MIN_SIZE, MAX_SIZE + 1)) / total if total else 0.0
                                 for r in range(1, top + 1)]}
    if keep:
        W = max((k[0].shape[1] for k in kept), default=MIN_SIZE)
        out["planted_rows"] = torch.cat([torch.nn.functional.pad(k[0], (0, W - k[0].shape[1])) for k in kept]) if kept else pos.new_zeros((0, W))
        out["planted"] = torch.cat([k[1] for k in kept]) if kept else torch.zeros(0, dtype=torch.int32, device=dev)
        out["order"] = torch.cat([k[2] for k in kept]) if kept else pos.new_zeros((0, top))
    return out


def report(result, log=print):
    """The reference's lines (History_version/Code/utils.py:229-232), per size and overall, with the chance level beside them."""
    for name, e in list(result["sizes"].items()) + [("all", result["overall"])]:
        for r in range(result["top"]):
            rate = e["hit"][r] / e["rows"] if e["rows"] else float("nan")
            log("size %s: outlier top %d hitting: %.4f (chance %.4f, %d rows)" % (name, r + 1, rate, e["chance"][r], e["rows"]))


def run(config: dict, model_path: str, sizes, top: int = 3, draws: int = 1, cycle: bool = False, seed: int = 0, device: str = "cuda", log=print):
    from .train import load_kmers
    sizes = sorted(int(k) for k in sizes)
    if sizes[0] < MIN_SIZE or sizes[-1] > MAX_SIZE:
        raise ValueError(f"--sizes must lie in {MIN_SIZE} .. {MAX_SIZE}")
    temp_dir = config["temp_dir"]
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy")).astype(np.int64)
    n2c_dict = np.load(os.path.join(temp_dir, "node2chrom.npy"), allow_pickle=True).item()
    N = int(sum(int(v[1] - v[0]) for v in chrom_range))
    node2chrom = np.full(N + 1, -1, dtype=np.int32)
    for k, v in n2c_dict.items():
        if 0 < int(k) <= N:
            node2chrom[int(k)] = int(v)
    model = torch.load(model_path, map_location=device, weights_only=False)                  # main.py:322, :685
    data, _ = load_kmers(temp_dir, sizes, float(config["quantile_cutoff_for_positive"]))
    known, _ = load_kmers(temp_dir, sizes, float(config["quantile_cutoff_for_unlabel"]))     # main.py:649-664
    dev = model.layer_norm1.weight.device
    hset = HyperedgeSet(torch.as_tensor(np.ascontiguousarray(known)).to(dev))
    pair_set = None
    if os.path.exists(os.path.join(temp_dir, "all_2_counter.npy")):
        pairs = np.load(os.path.join(temp_dir, "all_2_counter.npy")).astype(np.int64).reshape(-1, 2)
        pair_set = HyperedgeSet(torch.from_numpy(np.ascontiguousarray(pairs)).to(dev))
    planter = OutlierPlanter(hset, node2chrom, chrom_range.astype(np.int32), pair_set=pair_set, min_dis=int(config["min_distance"]), seed=seed)
    result = outlier_benchmark(model, data, planter, top=top, draws=draws, cycle=cycle)
    exhausted = planter.check_status()
    report(result, log)
    if exhausted:
        log("%d rows without a plant (256 trials exhausted): left out" % exhausted)
    return result


def main(argv=None):
    from . import utils as U
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="./config.JSON")
    ap.add_argument("--model", default=None, help="a pickled model (default: temp_dir/model2load)")
    ap.add_argument("--sizes", type=int, nargs="+", required=True, help="hyperedge sizes to plant in, 2 .. 32 (all_<k>_counter.npy of temp_dir)")
    ap.add_argument("--top", type=int, default=3, help="count the planted locus among the TOP least supported loci")
    ap.add_argument("--draws", type=int, default=1, help="planted copies per positive")
    ap.add_argument("--cycle", action="store_true", help="copy i replaces position i %% k instead of a drawn position")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    config = U.get_config(a.config)
    model_path = a.model or "model2load"
    if not os.path.exists(model_path):
        model_path = os.path.join(config["temp_dir"], model_path)
    run(config, model_path, a.sizes, a.top, a.draws, a.cycle, a.seed)


if __name__ == "__main__":
    main()
