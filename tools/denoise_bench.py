"""Cost of the denoised contact maps (csrc/denoise.hip + the quantile transforms) beside the pairwise sweep of the same chromosome.

  python tools/denoise_bench.py [--sizes 2491 24900] [--post-only] [--stats kernel_stats.csv]

For each n: the sweep (predict.pairwise_probabilities on a synthetic table model, d = 64, one chromosome of n bins) and the
post-processing (denoise.denoise_from_proba on a synthetic origin block), timed with device events after a warm-up; the host time of
tests/denoise_ref.py at n <= 2 491.  --post-only runs the post-processing alone (the run to put under rocprofv3 --kernel-trace --stats);
--stats reads that run's kernel_stats.csv and prints each stage's time with its algorithmic bytes and their fraction of the 6.3 TB/s
measured copy ceiling.  Algorithmic bytes, N = n^2 float32 elements: assembly 12N (proba and origin upper halves in, P and O out),
row sums and column sums 8N each for P and O and 4N each for my, combine 20N (P, O in; my_proba, origin_part, my out), finish 8N,
quantile transform kernel 8N per matrix (the radix sort's passes are on top), pixels 4N (half a matrix in and out); 92N with the sorts'
first read.
At n = 2 491 every matrix is 25 MB, below the 256 MiB Infinity Cache: that size is cache-resident, not an HBM measurement."""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import denoise as D
from matcha_amd import predict as PR
from matcha_amd import synth

COPY_CEILING = 6.3e12
STAGES = {   # kernel-name prefix -> (stage, bytes per matrix element)
    "denoise_assemble_kernel": ("assemble P, O", 12), "denoise_row_sums_kernel": ("row sums (P, O, my)", 12),
    "denoise_col_sums_kernel": ("column sums (P, O, my)", 12), "denoise_combine_kernel": ("combine", 20),
    "denoise_finish_kernel": ("finish my", 8), "denoise_pixels_kernel": ("pixels", 4),
    "quantile_transform_kernel": ("quantile transform x2", 16), "quantile_fit_kernel": ("quantile fit x2", 0),
}


def inputs(n, min_dis=2, seed=0):
    """proba U[0, 1) and origin U[0, 4) / (|i - j| + 1) with 1 % of the rows zeroed, made on the device."""
    g = torch.Generator("cuda").manual_seed(seed)
    proba = torch.rand(D.pair_count(n, min_dis), device="cuda", generator=g)
    idx = torch.arange(n, device="cuda", dtype=torch.float32)
    origin = torch.rand(n, n, device="cuda", generator=g) * 4.0 / ((idx[:, None] - idx[None, :]).abs() + 1.0)
    origin[torch.randperm(n, device="cuda", generator=g)[:max(1, n // 100)]] = 0.0
    return proba, origin


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def bench(n, post_only):
    min_dis = 2
    proba, origin = inputs(n, min_dis)
    post = timed(lambda: D.denoise_from_proba(proba, origin, n, min_dis), 5 if n < 10000 else 3)
    regime = "cache-resident (25 MB matrices)" if n * n * 4 < 256 << 20 else "HBM"
    line = f"n={n}: post-processing {post:.3f} ms ({regime}; {92 * n * n / (post * 1e-3) / 1e9:.0f} GB/s algorithmic, 92 bytes per element)"
    if not post_only:
        from tests.test_hip_model import hip_model
        clf, _ = hip_model([n, 16], 64, "table", 1)
        cr = np.asarray(synth.chrom_range([n, 16]))
        sweep = timed(lambda: PR.pairwise_probabilities(clf, cr, 0, min_dis), 2)
        line += f"; sweep {sweep:.1f} ms ({D.pair_count(n, min_dis) / sweep / 1e3:.1f} M pairs/s); post / sweep = {100 * post / sweep:.2f} %"
        if n <= 2491:
            from tests.denoise_ref import denoise_ref
            p, o = proba.cpu().numpy(), origin.cpu().numpy()
            t0 = time.perf_counter()
            denoise_ref(p, o, n, min_dis)
            line += f"; host numpy restatement {1e3 * (time.perf_counter() - t0):.0f} ms"
    print(line, flush=True)


def stats(path, n):
    """Per-stage times of a --post-only run at ONE size n (runs = launches of the assembly kernel)."""
    import csv
    rows = list(csv.DictReader(open(path)))
    runs = sum(int(r["Calls"]) for r in rows if "denoise_assemble_kernel" in r["Name"])
    print(f"per-stage kernel times at n={n} over {runs} runs ({path}); fraction of the {COPY_CEILING / 1e12:.1f} TB/s copy ceiling:")
    for r in rows:
        name, per_run = r["Name"], float(r["TotalDurationNs"]) / 1e6 / max(runs, 1)
        stage, per = next(((st, b) for k, (st, b) in STAGES.items() if k in name), ("radix sort (quantile)", 0)
                          if ("radix" in name.lower() or "rocprim" in name.lower()) else (None, 0))
        if stage is None:
            continue
        frac = f"{100 * per * n * n / (per_run * 1e-3) / COPY_CEILING:5.1f} %" if per else "    -  "
        print(f"  {stage:26s} {per_run:9.3f} ms/run  {per * n * n / 1e9:7.2f} GB  {frac}  [{name[:70]}]")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2491, 24900])
    ap.add_argument("--post-only", action="store_true")
    ap.add_argument("--stats", type=str, default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats, a.sizes[-1])
    else:
        for n in a.sizes:
            bench(n, a.post_only)
