"""Cost of cluster completion (matcha_amd/sweep.py::completion_sweep, kway_complete_rows_kernel) beside the eval forward
on the same rows.

  python tools/complete_bench.py [--reps 10] [--cases abc]

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process, as
tools/long_embedding_bench.py.  The partner region is chromosome 1 (its bins), min_gap 1, top 20:

  (a) 2 000 clusters of s uniform in [9, 25] ids, one free bin, width 26,
  (b) 200 clusters of 30 ids, two free bins, width 32,
  (c) 2 000 clusters of s uniform in [1, 7] ids, one free bin, width 8: the L <= 8 forward,

and per case, in the same run: the sweep; yardstick, model(x) alone over the same rows, generated beforehand, in the sweep's chunks and on
its route; and the rows kernel alone over all ranks in the sweep's chunks."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import _lib, synth  # noqa: E402
from matcha_amd import sweep as SW  # noqa: E402
from tools.long_bench import model, timed  # noqa: E402

CASES = {"a": (2000, (9, 25), 1, 26), "b": (200, (30, 30), 2, 32), "c": (2000, (1, 7), 1, 8)}       # clusters, sizes, free, width


def clusters_of(rng, N, A, sizes):
    t = np.zeros((A, sizes[1]), dtype=np.int64)
    for a, s in enumerate(rng.integers(sizes[0], sizes[1] + 1, size=A)):
        t[a, :s] = np.sort(rng.choice(N, size=int(s), replace=False) + 1)
    return t


def bench(reps, which):
    clf, _, num = model()
    N = int(np.sum(num))
    cr = np.asarray(synth.chrom_range(num))
    lo, hi = int(cr[0][0]), int(cr[0][1])
    n = hi - lo
    rng = np.random.default_rng(2027)
    print(f"region: {n} bins")
    print("| case | rows | chunk | sweep | model(x) on the same rows | rows kernel alone | sweep / model(x) | rows kernel / model(x) |")
    print("|---|---|---|---|---|---|---|---|")
    for name in which:
        A, sizes, free, width = CASES[name]
        table, _ = SW._cluster_table(clusters_of(rng, N, A, sizes), "cuda")
        total = SW.completion_count(A, table.shape[1], n, free, 1)
        chunk = min(total, 1 << 20 if width <= 8 else min(1 << 20, (1 << 21) // width))
        t_sweep = timed(lambda: SW.completion_sweep(clf, table, lo, hi, free=free, min_gap=1, top=20, width=width), reps)
        buf = torch.empty(chunk * width, dtype=torch.long, device="cuda")
        fbuf = torch.empty(chunk, dtype=torch.int32, device="cuda")

        def rows_only():
            for g0 in range(0, total, chunk):
                SW._complete_rows(table, lo, n, free, 1, g0, min(chunk, total - g0), None, width, buf, fbuf)

        t_rows = timed(rows_only, reps)
        x, _ = SW._complete_rows(table, lo, n, free, 1, 0, None, None, width, None, None)

        def forward_only():
            for g0 in range(0, total, chunk):
                clf(x[g0:g0 + chunk])

        with torch.no_grad(), clf.deferred_id_check(), _lib.option("disable_small_batch"):
            t_fwd = timed(forward_only, reps)
        del x, buf, fbuf
        torch.cuda.empty_cache()
        print(f"| ({name}) {A} clusters of {sizes[0]}..{sizes[1]}, free {free}, width {width} | {total} | {chunk} | {t_sweep:.2f} ms | {t_fwd:.2f} ms | "
              f"{t_rows:.3f} ms | {t_sweep / t_fwd:.3f} | {t_rows / t_fwd:.4f} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", type=str, default="abc")
    a = ap.parse_args()
    bench(a.reps, [c for c in a.cases if c in CASES])
