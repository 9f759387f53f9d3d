#!/usr/bin/env python3
"""Generate g11_kway_tiny.npz: the de novo k-way sweep's candidates scored by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and three (chromosome, k, min_gap) cases of the tiny
layout it stores

  rows_c<i>            the candidates, enumerated with itertools in lexicographic order (int64 [n, k]),
  logit_<mode>_c<i>    the logits of predict_multiway.py's own ``predict`` (:74-87) on them: one chunk, width k,
  ksel_<mode>_c<i>     the K in [10, 50) behind which the reference's sorted logits have their largest gap.

The gap at K_sel is asserted to be at least 100 x the project's tolerance (1e-4 of max |logit|), so the top-K_sel SET of the
reference is unambiguous for an implementation within that tolerance, and a test that compares sets at that K hides nothing.

Usage:  python tests/golden/make_golden_kway.py
"""
import io
import itertools
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import import_reference, redirect_stderr_null, ref_functions, synth  # noqa: E402

CASES = [(0, 3, 1), (2, 4, 2), (1, 5, 3)]          # (chromosome, k, min_gap) -> 560, 715, 56 candidates
TOL = 1e-4                                         # the project's tolerance against the reference's CPU logits
K_LO, K_HI = 10, 50


def enumerate_rows(lo, n, k, min_gap):
    rows = [c for c in itertools.combinations(range(lo, lo + n), k) if all(b - a >= min_gap for a, b in zip(c, c[1:]))]
    return np.asarray(rows, dtype=np.int64).reshape(-1, k)


def k_sel(logits):
    """(K, gap / max|logit|): the K in [K_LO, K_HI) with the largest gap between the K-th and the (K+1)-th sorted logit."""
    s = np.sort(logits.astype(np.float64))[::-1]
    gaps = s[K_LO - 1:K_HI - 1] - s[K_LO:K_HI]
    j = int(np.argmax(gaps))
    return K_LO + j, float(gaps[j] / np.abs(s).max())


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    cr = np.asarray(synth.chrom_range(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"cases": np.asarray(CASES, dtype=np.int64), "num": np.asarray(num, dtype=np.int64)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for i, (c, k, gap) in enumerate(CASES):
        lo, hi = int(cr[c][0]), int(cr[c][1])
        rows = enumerate_rows(lo, hi - lo, k, gap)
        out[f"rows_c{i}"] = rows
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                assert len(rows) <= 10000                              # one chunk of predict_multiway.py:77
                logits = np.asarray(pm["predict"](clf, rows)).reshape(-1).astype(np.float32)
            assert len(np.unique(logits)) == len(logits), "two candidates share a logit"
            K, gap_rel = k_sel(logits)
            assert gap_rel >= 100 * TOL, (c, k, gap, mode, K, gap_rel)
            out[f"logit_{mode}_c{i}"] = logits
            out[f"ksel_{mode}_c{i}"] = np.int64(K)
            print(f"case {i} (chrom {c}, k {k}, min_gap {gap}) {mode}: {len(rows)} rows, K_sel {K}, gap {gap_rel:.2e} of max|logit|")
    path = os.path.join(HERE, "g11_kway_tiny.npz")
    np.savez_compressed(path, **out)
    print("g11_kway_tiny.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
