#!/usr/bin/env python3
"""Generate g19_locus_scores.npz: the per-position scores of the REAL reference's classifier head.

Runs only in the build container (needs the reference; see make_golden.py and make_golden_long.py, whose helpers it imports and which it
does not change).  The reference's logit is the masked mean of ``pff_classifier((layer_norm1(dynamic) - layer_norm2(static))**2)`` of shape
[B, L, 1] (Modules.py:290-311); a forward hook on ``clf.pff_classifier`` captures that tensor while the reference's own ``clf(x)`` runs in
eval mode.  For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and every width L in {3, 8, 9, 17, 32} it stores

  rows_L<L>            8 rows of distinct ids of the 64-node tiny layout, zero-padded to L (int16 [8, L]): k = L, k = 2, then six rows of k
                       uniform in [2, L] (default_rng(SEED + L)); rows are sorted with trailing pads, except row ``moved_L<L>``, whose
                       FIRST id changed places with a pad: a zero inside the row,
  scores_<mode>_L<L>   float32 [8, L]   the hooked output, padding slots included (the reference masks them afterwards),
  logits_<mode>_L<L>   float32 [8]      clf(x)

(adj: np.random.seed(7) in front of each call; the draw only selects the reconstruction branch, which the logits do not depend on).

Usage:  python tests/golden/make_golden_locus_scores.py
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

WIDTHS = [3, 8, 9, 17, 32]
ROWS = 8
SEED = 1900


def make_rows(L, n_nodes):
    rng = np.random.default_rng(SEED + L)
    ks = [L, 2] + [int(k) for k in rng.integers(2, L + 1, size=ROWS - 2)]
    x = np.zeros((ROWS, L), dtype=np.int64)
    for i, k in enumerate(ks):
        x[i, :k] = np.sort(rng.choice(np.arange(1, n_nodes + 1), size=k, replace=False))
    # one zero inside a row: the first row behind the two fixed ones that has a pad gives its first id to its last column (none: row 1, k = 2)
    i = next((r for r in range(2, ROWS) if ks[r] < L), 1)
    x[i, L - 1], x[i, 0] = x[i, 0], 0
    return x, i


def main():
    torch.set_num_threads(4)
    import_reference()
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
            seen = []
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)
                clf.eval()
                hook = clf.pff_classifier.register_forward_hook(lambda mod, inp, res: seen.append(res.detach().clone()))
                np.random.seed(7)
                with torch.no_grad():
                    logits = clf(xt.clone())
                hook.remove()
            assert len(seen) == 1 and tuple(seen[0].shape) == (ROWS, L, 1), [tuple(s.shape) for s in seen]
            scores = seen[0].numpy().astype(np.float32).reshape(ROWS, L)
            logits = logits.detach().numpy().astype(np.float32).reshape(ROWS)
            assert np.isfinite(scores).all() and np.isfinite(logits).all()
            # the reference's own reduction of what the hook saw
            mask = (x != 0).astype(np.float32)
            assert np.allclose((scores * mask).sum(1) / (mask.sum(1) + 1e-15), logits, rtol=1e-5, atol=1e-6)
            out[f"scores_{mode}_L{L}"], out[f"logits_{mode}_L{L}"] = scores, logits
            print(f"L {L} {mode}: scores in [{scores.min():.4f}, {scores.max():.4f}], logits in [{logits.min():.4f}, {logits.max():.4f}]")
    path = os.path.join(HERE, "g19_locus_scores.npz")
    np.savez_compressed(path, **out)
    print("g19_locus_scores.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
