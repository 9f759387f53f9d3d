#!/usr/bin/env python3
"""Generate g15_complete_tiny.npz: cluster completion's candidates scored by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and the four cases of tests/complete_ref.py::G15_CASES
(chromosome, free, min_gap, width W, cluster sizes) it stores

  clusters_c<i>        the clusters, zero-padded (int16 [A, S]),
  rows_c<i>            every candidate of every cluster in global-rank order, zero-padded to W (int16 [A C_f, W]),
  valid_c<i>           the rule's verdict per candidate (bool [A C_f]),
  logit_<mode>_c<i>    the logits of predict_multiway.py's own ``predict`` (:74-87) on them, ONE chunk whose width is forced to W by one
                       filler row of W nodes (its logit is dropped): a logit depends on its chunk's width (SURVEY.md headline fact 7),
  ksel_<mode>_c<i>     per cluster the K_a in [2, min(8, valid - 1)] behind which the reference's sorted valid logits have their largest
                       gap (int64 [A]).

Asserted here: every logit of a cluster is distinct, and every such gap is >= 50 x the project's tolerance (1e-4) of the cluster's
max |logit| over its valid candidates, so the top-K_a SET of the reference is unambiguous for an implementation within that tolerance.

Usage:  python tests/golden/make_golden_complete.py
"""
import io
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import import_reference, redirect_stderr_null, ref_functions, synth  # noqa: E402
from tests import complete_ref as CR  # noqa: E402


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    n_nodes = int(np.sum(num))
    cr = np.asarray(synth.chrom_range(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"num": np.asarray(num, dtype=np.int64), "seed_base": np.int64(CR.G15_SEED)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    worst = {}
    for i, (c, free, gap, W, sizes) in enumerate(CR.G15_CASES):
        lo, hi = int(cr[c][0]), int(cr[c][1])
        clusters = CR.g15_clusters(i, n_nodes)
        assert [len(cl) for cl in clusters] == list(sizes) and max(sizes) + free <= W
        rows, bad = CR.table(clusters, lo, hi - lo, free, gap, W)
        cf = len(rows) // len(clusters)
        out[f"clusters_c{i}"] = CR.padded(clusters).astype(np.int16)
        out[f"rows_c{i}"] = rows.astype(np.int16)
        out[f"valid_c{i}"] = ~bad
        filler = list(range(1, W + 1))                                 # W nodes: pins the chunk's width
        samples = np.asarray([[int(v) for v in r if v != 0] for r in rows] + [filler], dtype=object)
        assert len(samples) <= 10000                                   # one chunk of predict_multiway.py:77
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                logits = np.asarray(pm["predict"](clf, samples)).reshape(-1).astype(np.float32)[:-1]
            assert logits.shape == (len(rows),) and np.isfinite(logits).all()
            ksel = []
            for a in range(len(clusters)):
                seg = slice(a * cf, (a + 1) * cf)
                lg, ok = logits[seg], ~bad[seg]
                assert len(np.unique(lg)) == len(lg), "two candidates of a cluster share a logit"
                K, g = CR.k_sel(lg[ok])
                rel = g / float(np.abs(lg[ok]).max())                      # the scale of logit_err on this cluster's kept rows
                assert rel >= 50 * CR.G15_TOL, (i, mode, a, K, rel)
                worst[i, mode] = min(worst.get((i, mode), np.inf), rel)
                ksel.append(K)
            out[f"logit_{mode}_c{i}"] = logits
            out[f"ksel_{mode}_c{i}"] = np.asarray(ksel, dtype=np.int64)
            print(f"case {i} (chrom {c}, free {free}, min_gap {gap}, W {W}) {mode}: {len(rows)} rows, valid per cluster "
                  f"{[int((~bad[a * cf:(a + 1) * cf]).sum()) for a in range(len(clusters))]}, K_a {ksel}, smallest gap {worst[i, mode]:.2e} of the cluster's max|logit|")
    path = os.path.join(HERE, "g15_complete_tiny.npz")
    np.savez_compressed(path, **out)
    print("g15_complete_tiny.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
