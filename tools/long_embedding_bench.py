"""Cost of Classifier.get_embedding on long rows (9 to 32 nodes: matcha_get_embedding_long, attn_long_prob_kernel) beside the eval
forward on the same input and beside writing a tensor of attn's size once.

  python tools/long_embedding_bench.py [--reps 10]
  python tools/long_embedding_bench.py --profile-only          (the run to put under rocprofv3 --kernel-trace --stats)
  python tools/long_embedding_bench.py --stats kernel_stats.csv

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process, as
tools/long_bench.py:

  (a) B = 10 000, L = 25, k uniform in [2, 25]: the reference's predict chunk,
  (b) B = 32 768, L = 32, k = 32: every slot real; attn is 1.07 GB,
  (c) B = 10 000, L = 25, 9 999 rows of k = 3 and one of k = 25: a chunk of short lines with one long one,

and per case, in the same run on code this tool's subject does not touch: yardstick 1, model(x) on the same input, and yardstick 2, a
device-to-device copy of a tensor of attn's size (32 B L^2 bytes), the floor for writing it once.  Reported: get_embedding, the forward,
their difference, and that difference in copies.  --profile-only runs get_embedding on (a), (b) and (c) three times each and nothing else;
--stats reads that run's kernel_stats.csv and prints every kernel's share."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from tools.long_bench import model, rows_of, stats, timed  # noqa: E402


def cases(N):
    rng = np.random.default_rng(2026)
    a = rows_of(rng, N, rng.integers(2, 26, size=10000), 25)
    b = np.concatenate([rows_of(rng, N, np.full(1 << 14, 32), 32) for _ in range(2)])
    kc = np.full(10000, 3)
    kc[6000] = 25
    return {"a": a, "b": b, "c": rows_of(rng, N, kc, 25)}


def bench(reps, profile_only):
    clf, _, num = model()
    cs = cases(int(np.sum(num)))
    what = {"a": "B 10 000, L 25, k uniform in [2, 25]", "b": "B 32 768, L 32, k 32", "c": "B 10 000, L 25, 9 999 rows of k 3 + one of k 25"}
    print("| case | attn | get_embedding | model(x) | difference | copy of attn's size | difference / copy |")
    print("|---|---|---|---|---|---|---|")
    with torch.no_grad(), clf.deferred_id_check():
        for name, x in cs.items():
            xt = torch.from_numpy(x).cuda()
            if profile_only:
                for _ in range(3):
                    clf.get_embedding(xt)
                torch.cuda.synchronize()
                continue
            B, L = x.shape
            t_emb = timed(lambda: clf.get_embedding(xt), reps)
            t_fwd = timed(lambda: clf(xt), reps)
            src = torch.empty(8 * B, L, L, dtype=torch.float32, device="cuda").normal_()
            dst = torch.empty_like(src)
            t_copy = timed(lambda: dst.copy_(src), reps)
            del src, dst
            torch.cuda.empty_cache()
            diff = t_emb - t_fwd
            print(f"| ({name}) {what[name]} | {32 * B * L * L / 1e6:.1f} MB | {t_emb:.3f} ms | {t_fwd:.3f} ms | {diff:.3f} ms | {t_copy:.3f} ms | "
                  f"{diff / t_copy:.2f} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--stats", type=str, default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        bench(a.reps, a.profile_only)
