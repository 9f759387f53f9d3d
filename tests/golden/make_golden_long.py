#!/usr/bin/env python3
"""Generate g12_long_rows.npz: rows of 9 to 32 nodes scored by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and every width L in {9, 12, 16, 17, 25, 32} it stores

  rows_L<L>            40 rows of distinct sorted ids of the 64-node tiny layout, zero-padded to L (int64 [40, L]): the first row has
                       k = L nodes, the second k = 2, the third k = 9, the others k uniform in [2, L] (default_rng(SEED + L)),
  logit_<mode>_L<L>    the logits of predict_multiway.py's own ``predict`` (:74-87) on them: one chunk, so the width is L.

A row's logit depends on its chunk's width (padding slots are attended keys, SURVEY.md headline fact 7): the first row pins the width.

Usage:  python tests/golden/make_golden_long.py
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
from make_golden import import_reference, redirect_stderr_null, ref_functions, synth  # noqa: E402

WIDTHS = [9, 12, 16, 17, 25, 32]
ROWS = 40
SEED = 1200


def make_rows(L, n_nodes):
    rng = np.random.default_rng(SEED + L)
    ks = [L, 2, 9] + [int(k) for k in rng.integers(2, L + 1, size=ROWS - 3)]
    return [np.sort(rng.choice(np.arange(1, n_nodes + 1), size=k, replace=False)).astype(np.int64) for k in ks]


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    n_nodes = int(np.sum(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"widths": np.asarray(WIDTHS, dtype=np.int64), "num": np.asarray(num, dtype=np.int64)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for L in WIDTHS:
        rows = make_rows(L, n_nodes)
        assert len(rows[0]) == L and len(rows) <= 10000                # one chunk of predict_multiway.py:77, padded to L
        padded = np.zeros((ROWS, L), dtype=np.int64)
        for i, r in enumerate(rows):
            padded[i, :len(r)] = r
        out[f"rows_L{L}"] = padded.astype(np.int16)
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                logits = np.asarray(pm["predict"](clf, np.asarray(rows, dtype=object))).reshape(-1).astype(np.float32)
            assert logits.shape == (ROWS,) and np.isfinite(logits).all()
            out[f"logit_{mode}_L{L}"] = logits
            print(f"L {L} {mode}: {ROWS} rows, logits in [{logits.min():.4f}, {logits.max():.4f}]")
    path = os.path.join(HERE, "g12_long_rows.npz")
    np.savez_compressed(path, **out)
    print("g12_long_rows.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
