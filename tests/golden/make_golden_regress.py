#!/usr/bin/env python3
"""Generate the gr_* fixtures of the regression task mode by running the REAL reference (main.py:60-117).

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
``forward_op_batch_regress`` is exec'd out of main.py's AST and called WITH ``y`` given: that path skips the sampler and the shuffle
(main.py:70-74), so a step is deterministic.  Dropout-free steps with torch.optim.AdamW(lr=1e-3) as main.py:630 builds it, the step's
loss ``loss * alpha + recon * beta`` as main.py:166 forms it.

Batches: mixed k, even B; pair j = rows (2j, 2j+1) of the reference's [B/2, 2] view is of category j % 5 -- pos-neg, neg-pos, neg-neg
(masked), pos-pos with equal weights (masked), pos-pos with distinct weights -- so every branch of the pair view, argmin and mask occurs.

Stored per step: x, y [B, 1], alpha, beta, the logits, softplus(logits), the MSE, the recon loss, the reference's pair outputs
(pred = sigmoid of the softplus difference, y = argmin label, s = size, masked pairs dropped); for step 0 which tensors have grad None
and every gradient element (every s-th element above ``CAP_GRAD`` elements: key grad0s<s>/name); the parameters after step 0 and after the
last step (above ``CAP_PARAM`` elements every s-th: param<step>[s<s>]/name).

Usage:  python tests/golden/make_golden_regress.py
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_ref, import_reference, main_functions, predraw_chroms, set_dropout, synth  # noqa: E402

CAP_GRAD, CAP_PARAM = 2048, 1024      # elements stored in full per tensor (every committed file stays under 1 MiB)
PHASE1, PHASE2 = (0.0, 1.0), (1.0, 0.001)       # main.py:637-638, :672-673


def regress_batch(rng, N, ks, rows_per_k):
    """x int64 [B, L] (mixed k, B even), y float32 [B, 1]: pair j of category j % 5 (see the module docstring)."""
    x, _, _ = synth.make_batch(rng, N, list(ks), rows_per_k)
    B = len(x) - len(x) % 2
    x = x[:B]
    y = np.zeros((B, 1), dtype=np.float32)
    for j in range(B // 2):
        w0, w1 = np.float32(round(rng.uniform(0.5, 4.0), 3)), np.float32(round(rng.uniform(0.5, 4.0), 3))
        if w1 == w0:
            w1 = np.float32(w0 + 0.25)
        c = j % 5
        if c == 0:
            y[2 * j, 0] = w0
        elif c == 1:
            y[2 * j + 1, 0] = w0
        elif c == 3:
            y[2 * j, 0] = y[2 * j + 1, 0] = w0
        elif c == 4:
            y[2 * j, 0], y[2 * j + 1, 0] = w0, w1
    return x, y


def _store(out, prefix, name, t, cap):
    """t in full up to `cap` elements (key prefix/name), else every s-th element of the flattened tensor (key prefix + s<s>/name)."""
    flat = t.reshape(-1)
    stride = -(-flat.size // cap)
    if stride == 1:
        out[f"{prefix}/{name}"] = t.copy()
    else:
        out[f"{prefix}s{stride}/{name}"] = flat[::stride].copy()


def gr_train(M, name, num, d, mode, seed, ks, rows_per_k, phases, caps=(CAP_GRAD, CAP_PARAM)):
    clf, attr, feats, inter_z, sd = build_ref(M, num, d, mode, seed)
    C, N = len(num), int(np.sum(num))
    set_dropout(clf, 0.0)
    clf.train()
    opt = torch.optim.AdamW(list(clf.parameters()), lr=1e-3, amsgrad=False)      # main.py:630
    glb = dict(F=torch.nn.functional, torch=torch, np=np, math=math)
    main_functions({"forward_op_batch_regress"}, glb)
    fwd = glb["forward_op_batch_regress"]
    brng = np.random.default_rng(seed + 7)
    n_steps = len(phases)
    out = {"alpha": np.asarray([a for a, _ in phases], dtype=np.float32), "beta": np.asarray([b for _, b in phases], dtype=np.float32)}
    batches = [regress_batch(brng, N, ks, rows_per_k) for _ in range(n_steps)]
    out["chroms"] = np.asarray(predraw_chroms(C, n_steps, 2345), dtype=np.int64)   # leaves numpy's stream where the forwards draw them
    logits_seen = []
    hook = clf.register_forward_hook(lambda m, i, o: logits_seen.append(o[0].detach().numpy().copy()))
    for step, ((x, y), (alpha, beta)) in enumerate(zip(batches, phases)):
        out[f"x{step}"] = x.astype(np.int16 if N < 32767 else np.int32)
        out[f"y{step}"] = y
        logits_seen.clear()
        pred, ly, loss, recon, w, s = fwd(clf, None, torch.from_numpy(x), torch.ones((len(x), 1)), torch.from_numpy(y))
        total = loss * alpha + recon * beta                                       # main.py:166
        opt.zero_grad()
        total.backward()
        z = logits_seen[-1]
        out[f"logits{step}"] = z
        out[f"sp{step}"] = torch.nn.functional.softplus(torch.from_numpy(z)).numpy()
        out[f"mse{step}"], out[f"recon{step}"] = loss.detach().numpy().copy(), recon.detach().numpy().copy()
        out[f"pair_pred{step}"], out[f"pair_y{step}"], out[f"pair_s{step}"] = (pred.detach().numpy().copy(), ly.numpy().copy(),
                                                                               s.numpy().copy())
        if step == 0:
            none = []
            for n_, p in clf.named_parameters():
                if p.grad is None:
                    none.append(n_)
                else:
                    _store(out, "grad0", n_, p.grad.numpy(), caps[0])
            out["grad_none"] = np.asarray(none)
        opt.step()
        if step in (0, n_steps - 1):
            for n_, p in clf.named_parameters():
                if not np.array_equal(p.detach().numpy(), np.asarray(sd[n_])):
                    _store(out, f"param{step}", n_, p.detach().numpy(), caps[1])
    hook.remove()
    path = os.path.join(HERE, f"gr_{name}.npz")
    np.savez_compressed(path, **out)
    print("GR", name, "rows", len(batches[0][0]), "mse0", out["mse0"], "recon0", out["recon0"], "pairs0", len(out["pair_y0"]),
          "bytes", os.path.getsize(path))


def main():
    torch.set_num_threads(4)
    M, _ = import_reference()
    K5 = (2, 3, 4, 5)
    tiny = [PHASE2, PHASE2, PHASE1, PHASE1]
    gr_train(M, "tiny_table", synth.LAYOUTS["tiny"], 64, "table", 101, (2, 3, 5), 20, tiny)      # 60 rows: the small-batch fused kernels
    gr_train(M, "tiny_adj", synth.LAYOUTS["tiny"], 64, "adj", 102, (2, 3, 5), 20, tiny)
    gr_train(M, "hg38_table_d64", synth.LAYOUTS["hg38_1mb"], 64, "table", 103, K5, 2304, [PHASE2, PHASE2])   # 9 216 rows
    gr_train(M, "hg38_adj_d64", synth.LAYOUTS["hg38_1mb"], 64, "adj", 104, K5, 2304, [PHASE2, PHASE2], caps=(768, 384))   # 23 adj encoders
    gr_train(M, "c1_table_d128", synth.LAYOUTS["c1"], 128, "table", 105, K5, 1024, [PHASE2, PHASE2])          # 4 096 rows (enc128)


if __name__ == "__main__":
    main()
