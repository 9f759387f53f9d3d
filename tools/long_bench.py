"""Cost of the inference forward for long rows (9 to 32 nodes: csrc/forward_long.hip, ragged_long.hip, attention_long.hip) beside the
L <= 8 forward and the CPU oracle.

  python tools/long_bench.py [--reps 10]
  python tools/long_bench.py --profile-only          (the run to put under rocprofv3 --kernel-trace --stats)
  python tools/long_bench.py --stats kernel_stats.csv

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process:

  (a) B = 10 000, L = 25, k uniform in [2, 25]: the reference's predict chunk (predict_multiway.py:77),
  (b) B = 2^17, L = 32, k = 32: every slot real,
  (c) B = 10 000, L = 25, 9 999 rows of k = 3 and one of k = 25: a chunk of short lines with one long one,

as rows/s and real tokens/s, and in the same run two yardsticks: the existing forward on rows of k = 8 at L = 8 with the same number of
real tokens as (a) and as (b), and the fp32 CPU oracle (oracle/hypersagnn.py, 16 threads) on (a).  --profile-only runs (a), (b) and (c)
three times each and nothing else; --stats reads that run's kernel_stats.csv and prints every kernel's share."""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import synth


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


def rows_of(rng, N, ks, L):
    """int64 [B, L]: row b holds ks[b] distinct sorted ids of 1..N, then zeros (vectorised: a random key per (row, node))."""
    ks = np.asarray(ks)
    order = np.argsort(rng.random((len(ks), N), dtype=np.float32), axis=1)[:, :L] + 1
    order[np.arange(L)[None, :] >= ks[:, None]] = N + 1                       # behind k: sorts to the end, then becomes padding
    x = np.sort(order, axis=1).astype(np.int64)
    x[x == N + 1] = 0
    return x


def cases(N):
    rng = np.random.default_rng(2025)
    a = rows_of(rng, N, rng.integers(2, 26, size=10000), 25)
    b = np.concatenate([rows_of(rng, N, np.full(1 << 14, 32), 32) for _ in range(8)])
    kc = np.full(10000, 3)
    kc[6000] = 25
    c = rows_of(rng, N, kc, 25)
    return {"a": a, "b": b, "c": c}


def model():
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    clf, sd = hip_model(num, 64, "table", 12)
    return clf.eval(), sd, num


def bench(reps, profile_only):
    clf, sd, num = model()
    N = int(np.sum(num))
    cs = cases(N)
    what = {"a": "B 10 000, L 25, k uniform in [2, 25]", "b": "B 2^17, L 32, k 32", "c": "B 10 000, L 25, 9 999 rows of k 3 + one of k 25"}
    tok_s = {}
    with torch.no_grad(), clf.deferred_id_check():
        for name, x in cs.items():
            xt = torch.from_numpy(x).cuda()
            if profile_only:
                for _ in range(3):
                    clf(xt)
                torch.cuda.synchronize()
                continue
            t = timed(lambda: clf(xt), reps)
            tokens = int((x != 0).sum())
            tok_s[name] = tokens / t / 1e3
            print(f"({name}) {what[name]}: {tokens} real tokens, {t:.3f} ms, {len(x) / t / 1e3:.3f} M rows/s, {tok_s[name]:.2f} M real tokens/s", flush=True)
        if profile_only:
            return
        # yardstick 1: the existing forward, rows of k = 8 at L = 8 with the same number of real tokens
        for name in ("a", "b"):
            tokens = int((cs[name] != 0).sum())
            B8 = tokens // 8
            x8 = torch.from_numpy(np.concatenate([rows_of(np.random.default_rng(8), N, np.full(min(B8 - r, 1 << 16), 8), 8) for r in range(0, B8, 1 << 16)])).cuda()
            t = timed(lambda: clf(x8), reps)
            short = 8 * B8 / t / 1e3
            print(f"L = 8 forward with the real tokens of ({name}): B {B8}, k 8: {t:.3f} ms, {B8 / t / 1e3:.3f} M rows/s, {short:.2f} M real tokens/s; "
                  f"long path / L = 8 path = {tok_s[name] / short:.3f} by tokens/s", flush=True)
    # yardstick 2: the fp32 CPU oracle on (a)
    from oracle import hypersagnn as O
    from tests.helpers import front_end
    torch.set_num_threads(16)
    P = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    fe = front_end(num, "table", 12)
    xa = torch.from_numpy(cs["a"])
    with torch.no_grad():
        O.classifier_forward(P, fe, xa[:512], random_chrom=0)
        t0 = time.perf_counter()
        O.classifier_forward(P, fe, xa, random_chrom=0)
        t = (time.perf_counter() - t0) * 1e3
    tokens = int((cs["a"] != 0).sum())
    print(f"fp32 CPU oracle on (a), 16 threads: {t:.1f} ms, {len(xa) / t / 1e3:.4f} M rows/s, {tokens / t / 1e3:.3f} M real tokens/s", flush=True)


def stats(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"kernel time of the profiled run ({path}): {total / 1e6:.2f} ms")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        print(f"  {ns / 1e6:9.3f} ms  {100 * ns / total:5.1f} %  {int(r['Calls']):5d} calls  {r['Name'][:100]}")


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
