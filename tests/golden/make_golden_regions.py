#!/usr/bin/env python3
"""Generate g18_regions_tiny.npz: the multi-region sweep's candidates scored by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports as make_golden_kway.py does, and
which it does not change).  For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and four cases of the tiny
layout (4 chromosomes of 16 bins) it stores

  parts_c<i>           int64 [P, 3]: (lo, hi, m) per part, in node ids,
  gap_c<i>             min_gap,
  valid_c<i>           uint8 [T]: 1 where every adjacent difference of the row is >= min_gap (0 only across a part boundary),
  ninvalid_c<i>        how many are 0,
  logit_<mode>_c<i>    the logits of predict_multiway.py's own ``predict`` (:74-87) on ALL T rows: one chunk, width k,
  ksel_<mode>_c<i>     the K in [10, 50) behind which the reference's sorted logits OF THE VALID ROWS have their largest gap.

The rows themselves are not stored: they are the per-part combinations under the gap rule (itertools.combinations), then their
product (itertools.product), in that order -- tests/regions_ref.py's ``candidates``, which the tests use too.  The gap at K_sel is
asserted to be at least 100 x the project's tolerance (1e-4 of max |logit|), as in make_golden_kway.py.

Three of the four cases were first asked for with other windows and failed that assertion on the adj model, so their windows were
moved, each keeping its parts' sizes, its m, its min_gap and its number of candidates:
  case 1  chr3[0, 8) -> chr3[8, 16)                         (adj: largest gap 0.89e-2 of max |logit| before, 1.54e-2 now)
  case 2  chr1[0, 6) x chr1[6, 16) -> chr2[0, 6) x chr2[6, 16)   (adj: 0.91e-2 before, 1.27e-2 now; 53 invalid rows either way)
  case 3  chr2[4, 10) -> chr2[6, 12)                        (adj: 0.92e-2 before, 1.26e-2 now)

Usage:  python tests/golden/make_golden_regions.py
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

sys.path.insert(0, ROOT)
from tests.regions_ref import CASES, candidates, case_parts  # noqa: E402  (the cases and the itertools enumeration, shared with the tests)

TOL = 1e-4
K_LO, K_HI = 10, 50


def k_sel(logits):
    s = np.sort(logits.astype(np.float64))[::-1]
    gaps = s[K_LO - 1:K_HI - 1] - s[K_LO:K_HI]
    j = int(np.argmax(gaps))
    return K_LO + j, float(gaps[j] / np.abs(s).max())


def main():
    sys.path.insert(0, HERE)
    from make_golden import import_reference, redirect_stderr_null, ref_functions, synth
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    cr = np.asarray(synth.chrom_range(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"num": np.asarray(num, dtype=np.int64), "n_cases": np.int64(len(CASES))}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for i, (case, gap) in enumerate(CASES):
        parts = case_parts(case, cr)
        rows, valid = candidates(parts, gap)
        out[f"parts_c{i}"] = np.asarray(parts, dtype=np.int64)
        out[f"gap_c{i}"] = np.int64(gap)
        out[f"valid_c{i}"] = valid.astype(np.uint8)
        out[f"ninvalid_c{i}"] = np.int64((~valid).sum())
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                assert len(rows) <= 10000                              # one chunk of predict_multiway.py:77
                logits = np.asarray(pm["predict"](clf, rows)).reshape(-1).astype(np.float32)
            assert len(np.unique(logits)) == len(logits), "two candidates share a logit"
            K, gap_rel = k_sel(logits[valid])
            assert gap_rel >= 100 * TOL, (i, mode, K, gap_rel)
            out[f"logit_{mode}_c{i}"] = logits
            out[f"ksel_{mode}_c{i}"] = np.int64(K)
            print(f"case {i} {mode}: {len(rows)} rows ({int((~valid).sum())} invalid), K_sel {K}, gap {gap_rel:.2e} of max|logit|")
    path = os.path.join(HERE, "g18_regions_tiny.npz")
    np.savez_compressed(path, **out)
    print("g18_regions_tiny.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
