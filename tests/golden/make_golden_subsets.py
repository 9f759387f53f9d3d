#!/usr/bin/env python3
"""Generate g16_subsets_tiny.npz: cluster decomposition's candidates scored by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and the five cases of tests/subsets_ref.py::G16_CASES
(mode, m, min_gap, width W, cluster sizes) it stores

  clusters_c<i>        the clusters, zero-padded (int16 [A, S_max]),
  rows_c<i>            every candidate, cluster after cluster, each cluster at its own size (S = s_a, as the sweep groups them) in rank
                       order, zero-padded to W (int16 [sum_a C(s_a, m), W]),
  offsets_c<i>         where each cluster's candidates begin (int64 [A + 1]),
  valid_c<i>           the rule's verdict per candidate (bool),
  logit_<mode>_c<i>    the logits of predict_multiway.py's own ``predict`` (:74-87) on them, ONE chunk whose width is forced to W by one
                       filler row of W nodes (its logit is dropped): a logit depends on its chunk's width (SURVEY.md headline fact 7),
  full_<mode>_c<i>     drop cases: the whole clusters' logits, scored in the same chunk (float32 [A]),
  ksel_<mode>_c<i>     per cluster the K_a in [2, min(8, valid - 1)] behind which the reference's sorted valid logits have their largest
                       gap (int64 [A]; complete_ref.k_sel),
  support_<mode>_c<i>  per cluster and locus the sum, in float64, of sigmoid(logit) over the valid candidates whose choice contains the
                       locus (float64 [A, S_max]).

Asserted here: every such gap is >= 50 x the project's tolerance (1e-4) of the cluster's max |logit| over its valid candidates, so the
top-K_a SET of the reference is unambiguous for an implementation within that tolerance.  Logits of one cluster need not be distinct.

Usage:  python tests/golden/make_golden_subsets.py
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
from tests import subsets_ref as SR  # noqa: E402


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    n_nodes = int(np.sum(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"num": np.asarray(num, dtype=np.int64), "seed_base": np.int64(SR.G16_SEED)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    worst = {}
    for i, (mode_name, m, gap, W, sizes) in enumerate(SR.G16_CASES):
        drop = mode_name == "drop"
        clusters = SR.g16_clusters(i, n_nodes)
        assert [len(cl) for cl in clusters] == list(sizes) and (max(sizes) if drop else m) <= W
        rows, bad, off = SR.g16_rows(i, clusters)
        A = len(clusters)
        out[f"clusters_c{i}"] = SR.padded(clusters).astype(np.int16)
        out[f"rows_c{i}"] = rows.astype(np.int16)
        out[f"offsets_c{i}"] = off
        out[f"valid_c{i}"] = ~bad
        lists = [[int(v) for v in r if v != 0] for r in rows] + ([list(cl) for cl in clusters] if drop else [])
        lists.append(list(range(1, W + 1)))                             # the filler, W nodes: pins the chunk's width
        if len({len(r) for r in lists}) == 1:                           # np2tensor_hyper rejects a uniform object array
            samples = np.asarray(lists, dtype=np.int64)
        else:
            samples = np.empty(len(lists), dtype=object)
            samples[:] = lists
        assert len(samples) <= 10000                                   # one chunk of predict_multiway.py:77
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                scored = np.asarray(pm["predict"](clf, samples)).reshape(-1).astype(np.float32)[:-1]
            assert scored.shape == (len(rows) + (A if drop else 0),) and np.isfinite(scored).all()
            logits = scored[:len(rows)]
            if drop:
                out[f"full_{mode}_c{i}"] = scored[len(rows):]
            ksel, sup = [], np.zeros((A, max(sizes)), dtype=np.float64)
            for a, cl in enumerate(clusters):
                seg = slice(int(off[a]), int(off[a + 1]))
                lg, ok = logits[seg], ~bad[seg]
                K, g = CR.k_sel(lg[ok])
                rel = g / float(np.abs(lg[ok]).max())                      # the scale of logit_err on this cluster's kept rows
                assert rel >= 50 * SR.G16_TOL, (i, mode, a, K, rel)
                worst[i, mode] = min(worst.get((i, mode), np.inf), rel)
                ksel.append(K)
                p = 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))
                for r, choice in enumerate(SR.choices(len(cl), m)):
                    if ok[r]:
                        sup[a, list(choice)] += p[r]
            out[f"logit_{mode}_c{i}"] = logits
            out[f"ksel_{mode}_c{i}"] = np.asarray(ksel, dtype=np.int64)
            out[f"support_{mode}_c{i}"] = sup
            print(f"case {i} ({mode_name}, m {m}, min_gap {gap}, W {W}) {mode}: {len(rows)} rows, valid per cluster "
                  f"{[int((~bad[off[a]:off[a + 1]]).sum()) for a in range(A)]}, K_a {ksel}, smallest gap {worst[i, mode]:.2e} of the cluster's max|logit|")
    path = os.path.join(HERE, "g16_subsets_tiny.npz")
    np.savez_compressed(path, **out)
    print("g16_subsets_tiny.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
