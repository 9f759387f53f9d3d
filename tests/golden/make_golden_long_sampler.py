#!/usr/bin/env python3
"""Generate sampler_stats_long.npz: statistics of the REAL reference's generate_negative (main.py:361-459) on rows of 9 to 25 nodes.

Runs only in the build container (needs the reference; see make_golden.py, whose reference import and ``main_functions`` it reuses and
which it does not change).  The case is the wide twin of make_golden.py::sampler_stats_c3: hg38 1 Mb (23 chromosomes), ONE mixed batch
with k in {9, 12, 16, 25} (ragged rows -> pad_sequence to 25), min_dis 0 and 2, neg_num 3, 1 000 positives per k out of 2 000 known per k
(tests/sampler_long_ref.py::long_sampler_case builds them; every positive has all adjacent gaps > min_dis, otherwise the reference never
returns).  Per min_dis and k it stores

  long_d<min_dis>_diff_k<k>   histogram of the number of nodes a negative differs from its positive in   (int64 [k + 1])
  long_d<min_dis>_pos_k<k>    histogram of WHICH position of the positive was replaced                     (int64 [k])

with the invariants of SURVEY.md 8 c3 asserted on the reference's output while the statistics are taken.

Usage:  python tests/golden/make_golden_long_sampler.py
"""
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import _RaggedNp, import_reference, main_functions, synth  # noqa: E402

sys.path.insert(0, ROOT)
from tests.sampler_long_ref import check_invariants, long_sampler_case, statistics  # noqa: E402

KS = (9, 12, 16, 25)
NEG_NUM = 3


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from pybloom_live import BloomFilter
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    cr, n2c = synth.chrom_range(num), synth.node2chrom(num)
    L = max(KS)
    out = {"ks": np.asarray(KS, dtype=np.int64)}
    for min_dis in (0, 2):
        batch, known, known_rows = long_sampler_case(min_dis, KS)
        dicts = [BloomFilter(10) for _ in range(L + 1)]
        for t in known:
            dicts[len(t)].add(t)
        glb = dict(train_dict=dicts, test_dict=dicts, max_size=L, min_size=2, node2chrom={i: int(n2c[i]) for i in range(1, N + 1)},
                   chrom_range=cr, min_dis=min_dis, task_mode="class", device=torch.device("cpu"), np=np, torch=torch,
                   math=math, random=random, np2tensor_hyper=U.np2tensor_hyper, pad_sequence=torch.nn.utils.rnn.pad_sequence)
        main_functions({"generate_negative", "neighbor_check"}, glb)
        ragged = np.empty(len(batch), dtype=object)
        for i, r in enumerate(batch):
            ragged[i] = r[r != 0]
        np.random.seed(16 + min_dis)
        random.seed(16 + min_dis)
        U.np = _RaggedNp()
        try:
            x, y, w, sizes = glb["generate_negative"](ragged, "train_dict", np.ones(len(ragged), dtype=np.float32), neg_num=NEG_NUM)
        finally:
            U.np = np
        x = x.numpy()
        P = len(batch)
        assert x.shape == ((1 + NEG_NUM) * P, L) and sizes.shape[0] == (1 + NEG_NUM) * P
        assert y[:P].min() == 1 and y[P:].max() == 0 and float(w[P:].min()) == 1.0
        assert np.array_equal(x[:P], batch)
        neg = x[P:]
        assert check_invariants(batch, neg, known, n2c, NEG_NUM, min_dis) == NEG_NUM * P
        diff, posh = statistics(batch, neg, NEG_NUM, KS)
        for k in KS:
            out[f"long_d{min_dis}_diff_k{k}"] = diff[k]
            out[f"long_d{min_dis}_pos_k{k}"] = posh[k]
            print("long sampler min_dis", min_dis, "k", k, "diff", diff[k], "positions", posh[k])
    np.savez_compressed(os.path.join(HERE, "sampler_stats_long.npz"), **out)


if __name__ == "__main__":
    main()
