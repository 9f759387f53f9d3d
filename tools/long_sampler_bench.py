#!/usr/bin/env python3
"""Time neg_sample_long_kernel (matcha_neg_sample_long: 32 lanes per negative) beside the unchanged neg_sample_kernel in one process.

  (a) the reference's step: 96 positives x 3 negatives at L = 25, k uniform in [9, 25], 4 000 known rows;
  (b) 16 384 positives x 3 at L = 32, k = 32, 400 000 known rows;
  yardstick: neg_sample_kernel at L = 8, k = 8 with the same number of negatives and known rows.

hg38 1 Mb layout (3 067 nodes), min_dis 0, every positive known (so every negative is redrawn).  Device events after a warm-up, the
median of --reps calls with the seed advancing as in training.  Prints negatives/s, ids/s (negatives x k) and the ratio to the yardstick
by negatives/s, then -- when the build's device assembly is there (build/csrc) -- the kernels' register counts and occupancy.

Usage:  python tools/long_sampler_bench.py [--reps 10]
"""
import argparse
import glob
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from matcha_amd import synth  # noqa: E402
from matcha_amd.sampler import HyperedgeSet, NegativeSampler  # noqa: E402


def time_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def case(label, N, n2c, cr, known, P, reps):
    """known int64 [M, L] on the device; the first P rows are the positives."""
    hs = HyperedgeSet(known)
    smp = NegativeSampler(hs, n2c, cr, neg_num=3, min_dis=0, seed=1)
    pos = known[:P].contiguous()
    out = torch.empty(P * 3, known.shape[1], dtype=torch.long, device="cuda")
    ms = time_ms(lambda: smp.sample_into(pos, out), reps)
    exhausted = smp.check_status()
    ids = int((pos != 0).sum()) * 3
    assert not torch.equal(out, pos.repeat_interleave(3, dim=0))
    print(f"{label}: {P * 3} negatives, {ids} ids, {len(known)} known rows, {ms * 1e3:.1f} us, {P * 3 / ms / 1e3:.3f} M negatives/s, "
          f"{ids / ms / 1e3:.2f} M ids/s, exhausted {exhausted}")
    return P * 3 / ms


def kernel_stats():
    files = glob.glob(os.path.join(ROOT, "build", "csrc", "sampler-hip-amdgcn-amd-amdhsa-*.s"))
    if not files:
        print("register counts: build/csrc has no device assembly here (it is written by the build)")
        return
    src = open(files[0]).read()
    for name in ("neg_sample_long_kernel", "neg_sample_kernel"):
        m = re.search(r"\.set _ZN6matcha%d%sE\w*\.has_indirect_call.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)" % (len(name), name), src, re.S)
        if m:
            print(f"{name}: {m.group(1)} VGPRs, scratch {m.group(2)} B, occupancy {m.group(3)} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    rng = np.random.default_rng(0)
    ka = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, 240), ((0, 0), (0, 25 - k))) for k in range(9, 26)])
    ka = torch.from_numpy(ka[rng.permutation(len(ka))]).cuda()                                   # 4 080 rows, k uniform in [9, 25]
    a_long = case("(a) L 25, k uniform in [9, 25], neg_sample_long_kernel", N, n2c, cr, ka, 96, a.reps)
    y8 = torch.from_numpy(synth.make_edges_fast(rng, N, 8, len(ka))).cuda()
    a_short = case("    yardstick L 8, k 8, neg_sample_kernel", N, n2c, cr, y8, 96, a.reps)
    print(f"    (a) / yardstick by negatives/s: {a_long / a_short:.3f}")
    kb = torch.unique(synth.make_edges_device(N, 400000, ks=(32,), seed=5), dim=0)
    kb = kb[torch.randperm(len(kb), device="cuda", generator=torch.Generator("cuda").manual_seed(1))]
    b_long = case("(b) L 32, k 32, neg_sample_long_kernel", N, n2c, cr, kb, 16384, a.reps)
    y8b = torch.unique(synth.make_edges_device(N, 400000, ks=(8,), seed=6), dim=0)
    y8b = y8b[torch.randperm(len(y8b), device="cuda", generator=torch.Generator("cuda").manual_seed(2))]
    b_short = case("    yardstick L 8, k 8, neg_sample_kernel", N, n2c, cr, y8b, 16384, a.reps)
    print(f"    (b) / yardstick by negatives/s: {b_long / b_short:.3f}")
    kernel_stats()


if __name__ == "__main__":
    main()
