#!/usr/bin/env python3
"""Generate g13_long_grads.npz: one training step on rows of 9 and of 32 nodes by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}), every nn.Dropout.p set to 0, train mode, and each width
L in {9, 32} it stores

  x_L<L>, y_L<L>, w_L<L>         24 rows of distinct sorted ids of the 64-node tiny layout, zero-padded to L: the first rows have k = L, 2, 1, 9
                                 nodes, the others k uniform in [2, L] (default_rng(SEED + L)); labels in {0, 1}, weights in [0.5, 2),
  chrom_<mode>_L<L>              the random_chrom the forward drew (np.random.seed(NP_SEED + L), Modules.py:192),
  logits / bce / recon _<mode>_L<L>   of loss = bce * 1 + recon * 0.001 (main.py:56),
  grad_<mode>_L<L>/<name>        every parameter's gradient after loss.backward(), and none_<mode>_L<L> the names whose .grad is None.

Usage:  python tests/golden/make_golden_long_grads.py
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, predraw_chroms, redirect_stderr_null, set_dropout, synth  # noqa: E402

WIDTHS = [9, 32]
ROWS = 24
SEED = 1300
NP_SEED = 4300


def make_batch(L, n_nodes):
    rng = np.random.default_rng(SEED + L)
    ks = [L, 2, 1, 9] + [int(k) for k in rng.integers(2, L + 1, size=ROWS - 4)]
    x = np.zeros((ROWS, L), dtype=np.int64)
    for b, k in enumerate(ks):
        x[b, :k] = np.sort(rng.choice(np.arange(1, n_nodes + 1), size=k, replace=False))
    y = (rng.random((ROWS, 1)) < 0.5).astype(np.float32)
    w = (0.5 + 1.5 * rng.random((ROWS, 1))).astype(np.float32)
    return x, y, w


def main():
    torch.set_num_threads(4)
    import_reference()
    num = synth.LAYOUTS["tiny"]
    n_nodes, C = int(np.sum(num)), len(num)
    out = {"widths": np.asarray(WIDTHS, dtype=np.int64), "num": np.asarray(num, dtype=np.int64)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for L in WIDTHS:
        x, y, w = make_batch(L, n_nodes)
        out[f"x_L{L}"], out[f"y_L{L}"], out[f"w_L{L}"] = x.astype(np.int16), y, w
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
            set_dropout(clf, 0.0)
            clf.train()
            tag = f"{mode}_L{L}"
            out[f"chrom_{tag}"] = np.int64(predraw_chroms(C, 1, NP_SEED + L)[0])       # leaves the seed where the forward expects it
            pred, recon = clf(torch.from_numpy(x), return_recon=True)
            bce = torch.nn.functional.binary_cross_entropy_with_logits(pred, torch.from_numpy(y), weight=torch.from_numpy(w))
            (bce * 1.0 + recon * 0.001).backward()
            out[f"logits_{tag}"] = pred.detach().numpy().reshape(-1).copy()
            out[f"bce_{tag}"] = np.float32(bce.detach())
            out[f"recon_{tag}"] = np.float32(recon.detach().reshape(-1)[0])
            none = []
            for n_, p in clf.named_parameters():
                if p.grad is None:
                    none.append(n_)
                else:
                    out[f"grad_{tag}/{n_}"] = p.grad.numpy().copy()
            out[f"none_{tag}"] = np.asarray(none)
            print(f"L {L} {mode}: bce {float(bce):.5f} recon {float(out[f'recon_{tag}']):.5f} chrom {int(out[f'chrom_{tag}'])} none {len(none)}")
    path = os.path.join(HERE, "g13_long_grads.npz")
    np.savez_compressed(path, **out)
    print("g13_long_grads.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
