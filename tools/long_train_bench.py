"""Cost of a training step on long rows (9 to 32 nodes: matcha_forward_long_train / matcha_backward_long, attention_long_bwd.hip) beside the
L <= 8 steps, all through the same surface: model(x), a weighted BCE in torch, loss.backward().

  python tools/long_train_bench.py [--reps 10]
  python tools/long_train_bench.py --profile-only          (the run to put under rocprofv3 --kernel-trace --stats)
  python tools/long_bench.py --stats kernel_stats.csv      (reads that run's statistics)

d = 64 table model, hg38 at 1 Mb, train mode with the model's own dropout, model.long_row_training = True, forward + backward timed with
device events after a warm-up (median of --reps), one process:

  (a) B = 10 000, L = 25, k uniform in [2, 25],
  (b) B = 2^15, L = 32, k = 32: every slot real,

as rows/s and real tokens/s, and in the same run two yardsticks on rows of k = 8 at L = 8 with the same number of real tokens: the
layer-by-layer step (option disable_fused = 1: the chain the long step shares everything but the plan and the attention with) and the
fused step.  --profile-only runs (a) and (b) three times each and nothing else."""
import argparse
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from matcha_amd import _lib, synth
from tools.long_bench import rows_of, timed


def cases(N):
    rng = np.random.default_rng(2026)
    a = rows_of(rng, N, rng.integers(2, 26, size=10000), 25)
    b = np.concatenate([rows_of(rng, N, np.full(1 << 14, 32), 32) for _ in range(2)])
    return {"a": a, "b": b}


def model():
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    clf, _ = hip_model(num, 64, "table", 12)
    clf.long_row_training = True
    return clf.train(), num


def batch(x):
    rng = np.random.default_rng(len(x))
    y = torch.from_numpy((rng.random((len(x), 1)) < 0.5).astype(np.float32)).cuda()
    w = torch.from_numpy((0.5 + 1.5 * rng.random((len(x), 1))).astype(np.float32)).cuda()
    return torch.from_numpy(x).cuda(), y, w


def bench(reps, profile_only):
    clf, num = model()
    N = int(np.sum(num))
    cs = cases(N)
    what = {"a": "B 10 000, L 25, k uniform in [2, 25]", "b": "B 2^15, L 32, k 32"}

    def fb(xt, y, w):
        for p in clf.parameters():
            p.grad = None
        F.binary_cross_entropy_with_logits(clf(xt), y, weight=w).backward()

    tok_s = {}
    with clf.deferred_id_check():
        for name, x in cs.items():
            xt, y, w = batch(x)
            if profile_only:
                for _ in range(3):
                    fb(xt, y, w)
                torch.cuda.synchronize()
                continue
            t = timed(lambda: fb(xt, y, w), reps)
            tokens = int((x != 0).sum())
            tok_s[name] = tokens / t / 1e3
            print(f"({name}) {what[name]}: {tokens} real tokens, {t:.3f} ms, {len(x) / t / 1e3:.3f} M rows/s, {tok_s[name]:.2f} M real tokens/s", flush=True)
        if profile_only:
            return
        for label, option in (("layer-by-layer (disable_fused = 1)", "disable_fused"), ("fused", None)):
            for name in ("a", "b"):
                tokens = int((cs[name] != 0).sum())
                B8 = tokens // 8
                x8 = np.concatenate([rows_of(np.random.default_rng(8), N, np.full(min(B8 - r, 1 << 16), 8), 8) for r in range(0, B8, 1 << 16)])
                xt, y, w = batch(x8)
                if option:
                    with _lib.option(option):
                        t = timed(lambda: fb(xt, y, w), reps)
                else:
                    t = timed(lambda: fb(xt, y, w), reps)
                short = 8 * B8 / t / 1e3
                print(f"L = 8 {label} step with the real tokens of ({name}): B {B8}, k 8: {t:.3f} ms, {B8 / t / 1e3:.3f} M rows/s, "
                      f"{short:.2f} M real tokens/s; long step / this = {tok_s[name] / short:.3f} by tokens/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    bench(a.reps, a.profile_only)
