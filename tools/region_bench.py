"""Cost of the multi-region sweep (matcha_amd/sweep.py::region_sweep / region_map, csrc/sweep_rows.hip::kway_region_rows_kernel)
beside the eval forward on the same rows, and of its rows kernel beside kway_rows_kernel.

  python tools/region_bench.py [--reps 10] [--cases ab]

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process, as
tools/grow_bench.py.  min_gap 1, chunks of 2^20 rows, top 1 000:

  (a) k = 3: one bin from each of chromosomes 1, 6 and 11 (whole chromosomes),
  (b) k = 4: one bin of chr1[0, 100), two of chr6[0, 100), one of chr11[0, 10),

and per case, in the same run: region_sweep; region_map between the first and the last part; yardstick (DESIGN.md 7.3's), model(x) alone
over the same rows, generated beforehand, in the sweep's chunks and on its route; the region rows kernel alone over the same chunks; and
kway_rows_kernel alone at the same count, chunks and width (the first T ranks of a one-region sweep of the same k)."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import _lib, synth  # noqa: E402
from matcha_amd import sweep as SW  # noqa: E402
from tools.long_bench import model, timed  # noqa: E402

CHUNK, TOP = 1 << 20, 1000


def cases(cr):
    c = lambda i, a=None, b=None: (int(cr[i][0]) + (a or 0), int(cr[i][0]) + b if b is not None else int(cr[i][1]))
    return {"a": ([c(0) + (1,), c(5) + (1,), c(10) + (1,)], (1, 400, 3)),
            "b": ([c(0, 0, 100) + (1,), c(5, 0, 100) + (2,), c(10, 0, 10) + (1,)], (1, 120, 4))}


def bench(reps, which):
    clf, _, num = model()
    cr = np.asarray(synth.chrom_range(num))
    print("| case | candidates | region_sweep | region_map | model(x) on the same rows | region rows alone | kway_rows alone | sweep / model(x) | "
          "map / model(x) | region rows / model(x) | region rows / kway_rows |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name in which:
        parts, (klo, kn, kk) = cases(cr)[name]
        k = sum(m for _, _, m in parts)
        T = SW.region_count(parts, 1)
        assert kk == k and SW.kway_count(kn, kk, 1) >= T
        last = len(parts) - 1
        t_sweep = timed(lambda: SW.region_sweep(clf, parts, 1, top=TOP, chunk_rows=CHUNK), reps)
        t_map = timed(lambda: SW.region_map(clf, parts, 1, 0, last, chunk_rows=CHUNK), reps)
        xs = [SW.region_rows(parts, 1, rank0=g0, count=min(CHUNK, T - g0))[0] for g0 in range(0, T, CHUNK)]

        def forward_only():
            for x in xs:
                clf(x)

        with torch.no_grad(), clf.deferred_id_check(), _lib.option("disable_small_batch"):
            t_fwd = timed(forward_only, reps)
        del xs
        buf = torch.empty(CHUNK * k, dtype=torch.long, device="cuda")
        fbuf = torch.empty(CHUNK, dtype=torch.int32, device="cuda")

        def region_rows_only():
            for g0 in range(0, T, CHUNK):
                SW.region_rows(parts, 1, rank0=g0, count=min(CHUNK, T - g0), out=buf, flag_out=fbuf)

        def kway_rows_only():
            for g0 in range(0, T, CHUNK):
                SW.kway_rows(klo, kn, kk, 1, rank0=g0, count=min(CHUNK, T - g0), out=buf)

        t_rr = timed(region_rows_only, reps)
        t_kr = timed(kway_rows_only, reps)
        torch.cuda.empty_cache()
        shape = " x ".join("%d bins, m = %d" % (hi - lo, m) for lo, hi, m in parts)
        print(f"| ({name}) k = {k}: {shape} | {T} | {t_sweep:.2f} ms | {t_map:.2f} ms | {t_fwd:.2f} ms | {t_rr:.3f} ms | {t_kr:.3f} ms | "
              f"{t_sweep / t_fwd:.3f} | {t_map / t_fwd:.3f} | {t_rr / t_fwd:.4f} | {t_rr / t_kr:.2f} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", type=str, default="ab")
    a = ap.parse_args()
    bench(a.reps, [c for c in a.cases if c in "ab"])
