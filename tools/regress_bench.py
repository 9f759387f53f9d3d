"""Same-process A/B of the two training objectives (development tool): Trainer(objective="class") against Trainer(objective="regress")
at the headline shape (hg38 1 Mb, table front end, embed_dim 64, 65 536 rows) and at the reference's 192-row regress step (96 positives
+ 96 negatives), each eager (Trainer.step per iteration) and as a hipGraph replay (Trainer.capture).  Windows alternate between the two
objectives; the median per-step time of each is printed as one JSON line, with the time of the two epochs' per-step bookkeeping
kernels (matcha_step_record, matcha_step_record_pairs) at the same row counts.

    python tools/regress_bench.py [--steps 50] [--windows 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from matcha_amd import synth  # noqa: E402
from matcha_amd.engine import Trainer  # noqa: E402


def model(num, d, seed):
    import Modules as M
    from oracle import hypersagnn as O
    attr = O.attribute_table(num)
    sd = synth.make_state_dict(np.random.default_rng(seed), num, d, "table", attr)
    N = int(np.sum(num))
    clf = M.Classifier(n_head=8, d_model=d, d_k=d, d_v=d, node_embedding=M.Wrap_Embedding(N + 1, d, padding_idx=0), diag_mask=True,
                       bottle_neck=d, attribute_dict=attr)
    clf.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return clf.to("cuda").train()


def batch(rng, N, rows, regress):
    x, y, w = synth.make_batch(rng, N, [2, 3, 4, 5], rows // 4 + 1)
    x, y, w = x[:rows], y[:rows].reshape(-1), w[:rows].reshape(-1)
    if regress:
        y = np.where(np.arange(rows) % 2 == 0, w, 0.0).astype(np.float32)
        w = np.ones(rows, dtype=np.float32)
    return (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))


def time_window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    out = {}
    for rows in (65536, 192):
        runners = {}
        for objective in ("class", "regress"):
            clf = model(num, 64, 3)
            tr = Trainer(clf, lr=1e-3, objective=objective)
            x, y, w = batch(np.random.default_rng(rows), N, rows, objective == "regress")
            runners[(objective, "eager")] = (lambda tr=tr, x=x, y=y, w=w: tr.step(x, y, w, 1.0, 0.001))
            runners[(objective, "graph")] = tr.capture(x, y, w, 1.0, 0.001)
        for fn in runners.values():
            time_window(fn, 3)                                   # warm-up
        ms = {k: [] for k in runners}
        for _ in range(a.windows):
            for k, fn in runners.items():                        # interleaved windows: drift hits both objectives alike
                ms[k].append(time_window(fn, a.steps))
        for (objective, how), v in ms.items():
            out[f"{rows}_{how}_{objective}_ms"] = float(np.median(v))
        for how in ("eager", "graph"):
            out[f"{rows}_{how}_regress_over_class"] = out[f"{rows}_{how}_regress_ms"] / out[f"{rows}_{how}_class_ms"]
    # the regress epoch's per-step bookkeeping (matcha_step_record_pairs) against the class epoch's (matcha_step_record), same rows
    import ctypes as C
    from matcha_amd import _lib
    lib = _lib.load()
    for rows in (65536, 192):
        x, y, _ = batch(np.random.default_rng(rows), N, rows, True)
        lg = torch.randn(rows, device="cuda")
        losses, sums = torch.zeros(3, device="cuda"), torch.zeros(2, device="cuda")
        it, seed = torch.zeros(1, dtype=torch.long, device="cuda"), torch.ones(1, dtype=torch.long, device="cuda")
        n = a.steps
        preds, sizes = torch.empty((n, rows), device="cuda"), torch.empty((n, rows), dtype=torch.long, device="cuda")
        pl = torch.empty((n, rows // 2), dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L = int(x.shape[1])
        rec = {"record": lambda: lib.matcha_step_record(_lib.ptr(lg), _lib.ptr(losses), _lib.ptr(x), rows, L, _lib.ptr(it), n, _lib.ptr(sums),
                                                         _lib.ptr(preds), _lib.ptr(sizes), st),
               "record_pairs": lambda: lib.matcha_step_record_pairs(_lib.ptr(lg), _lib.ptr(losses), _lib.ptr(y), _lib.ptr(x), rows, L, _lib.ptr(it),
                                                                    n, _lib.ptr(seed), _lib.ptr(sums), _lib.ptr(preds), _lib.ptr(pl),
                                                                    _lib.ptr(sizes), st)}
        for k, fn in rec.items():
            time_window(fn, 3)
            out[f"{rows}_{k}_us"] = 1e3 * float(np.median([time_window(fn, a.steps) for _ in range(a.windows)]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
