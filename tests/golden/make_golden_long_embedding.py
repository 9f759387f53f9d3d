#!/usr/bin/env python3
"""Generate g14_long_embedding.npz: Classifier.get_embedding of the REAL reference on rows of 9 to 32 columns.

Runs only in the build container (needs the reference; see make_golden.py and make_golden_long.py, whose helpers it imports and which it
does not change).  For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and every width L in {9, 17, 32} it stores

  rows_L<L>              8 rows of distinct ids of the 64-node tiny layout, zero-padded to L (int16 [8, L]): k = L, 2, 9, then five rows of
                         k uniform in [2, L] (default_rng(SEED + L)); rows are sorted with trailing pads, except row 4, whose FIRST id
                         changed places with a pad: a zero inside the row,
  dynamic_<mode>_L<L>    float32 [8, L, 16]
  static_<mode>_L<L>     float32 [8, L, 16]
  attn_<mode>_L<L>       float32 [64, L, L]   (index h * 8 + b)

-- the reference's own get_embedding(x, get_attn_key_pad_mask(x, x), get_non_pad_mask(x)) in eval mode (adj: np.random.seed(7) in front of
each call; the draw only selects the reconstruction branch, which get_embedding does not return).

Usage:  python tests/golden/make_golden_long_embedding.py
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_long import import_reference, redirect_stderr_null, synth  # noqa: E402

WIDTHS = [9, 17, 32]
ROWS = 8
SEED = 1400


def make_rows(L, n_nodes):
    rng = np.random.default_rng(SEED + L)
    ks = [L, 2, 9] + [int(k) for k in rng.integers(2, L + 1, size=ROWS - 3)]
    x = np.zeros((ROWS, L), dtype=np.int64)
    for i, k in enumerate(ks):
        x[i, :k] = np.sort(rng.choice(np.arange(1, n_nodes + 1), size=k, replace=False))
    # one zero inside a row: row 4's first id goes to the row's last column (if the row is full, row 1 -- k = 2 -- takes its place)
    i = 4 if ks[4] < L else 1
    x[i, L - 1], x[i, 0] = x[i, 0], 0
    return x, i


def main():
    torch.set_num_threads(4)
    M, _ = import_reference()
    num = synth.LAYOUTS["tiny"]
    n_nodes = int(np.sum(num))
    out = {"widths": np.asarray(WIDTHS, dtype=np.int64), "num": np.asarray(num, dtype=np.int64)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for L in WIDTHS:
        x, moved = make_rows(L, n_nodes)
        out[f"rows_L{L}"] = x.astype(np.int16)
        out[f"moved_L{L}"] = np.asarray(moved, dtype=np.int64)
        xt = torch.from_numpy(x)
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                clf.eval()
                np.random.seed(7)
                with torch.no_grad():
                    dyn, sta, attn = clf.get_embedding(xt.clone(), M.get_attn_key_pad_mask(xt, xt), M.get_non_pad_mask(xt))
            dyn, sta, attn = (t.detach().numpy().astype(np.float32) for t in (dyn, sta, attn))
            assert dyn.shape == sta.shape == (ROWS, L, 16) and attn.shape == (8 * ROWS, L, L)
            assert np.isfinite(dyn).all() and np.isfinite(sta).all() and np.isfinite(attn).all()
            out[f"dynamic_{mode}_L{L}"], out[f"static_{mode}_L{L}"], out[f"attn_{mode}_L{L}"] = dyn, sta, attn
            print(f"L {L} {mode}: attn in [{attn.min():.3e}, {attn.max():.4f}], |dynamic| <= {np.abs(dyn).max():.4f}")
    path = os.path.join(HERE, "g14_long_embedding.npz")
    np.savez_compressed(path, **out)
    print("g14_long_embedding.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
