"""Cost of cluster growth (matcha_amd/sweep.py::growth_sweep, csrc/grow.hip) beside the eval forward on the same rows and
beside cluster completion called step by step.

  python tools/grow_bench.py [--reps 10] [--cases ab]

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process, as
tools/complete_bench.py.  The region is chromosome 1 (its bins), min_gap 1, beam 8:

  (a) 200 single-locus seeds, max_size 8, width 8: the L <= 8 forward,
  (b) 200 seeds of 9 loci, max_size 20, width 20: the long forward,

and per case, in the same run: growth_sweep; yardstick, model(x) alone over the same rows of every step, generated beforehand, in the
sweep's chunks and on its route; completion_sweep(free=1, top=8) called once per step on the same beams (what there was before: a
read-back per step, no merge across a seed's slots, no twins); and the two growth kernels alone over all steps."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import _lib, synth  # noqa: E402
from matcha_amd import sweep as SW  # noqa: E402
from tools.long_bench import model, timed  # noqa: E402

CASES = {"a": (200, 1, 8, 8), "b": (200, 9, 20, 20)}                      # seeds, seed size, max_size, width
BEAM = 8


def bench(reps, which):
    clf, _, num = model()
    N = int(np.sum(num))
    cr = np.asarray(synth.chrom_range(num))
    lo, hi = int(cr[0][0]), int(cr[0][1])
    n = hi - lo
    rng = np.random.default_rng(2028)
    print(f"region: {n} bins")
    print("| case | steps | rows | growth_sweep | model(x) on the same rows | completion_sweep per step | twins + flags alone | growth / model(x) | "
          "growth / completion steps | kernels / model(x) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in which:
        A, s, max_size, width = CASES[name]
        seeds = np.stack([np.sort(rng.choice(N, size=s, replace=False) + 1) for _ in range(A)])
        beams, inner = [], SW._grow_step

        def recording(model_, beam, *args):
            beams.append(beam.clone())
            return inner(model_, beam, *args)

        SW._grow_step = recording                                        # the beams that enter every step, once
        out = SW.growth_sweep(clf, seeds, lo, hi, max_size, beam=BEAM, width=width)
        SW._grow_step = inner
        assert len(beams) == out["steps"] == max_size - s
        t_grow = timed(lambda: SW.growth_sweep(clf, seeds, lo, hi, max_size, beam=BEAM, width=width), reps)
        chunk = 1 << 20 if width <= 8 else min(1 << 20, (1 << 21) // width)
        xs = [SW._complete_rows(b.view(-1, b.shape[2]), lo, n, 1, 1, 0, None, None, width, None, None)[0] for b in beams]
        rows = sum(int(x.shape[0]) for x in xs)

        def forward_only():
            for x in xs:
                for g0 in range(0, int(x.shape[0]), chunk):
                    clf(x[g0:g0 + chunk])

        with torch.no_grad(), clf.deferred_id_check(), _lib.option("disable_small_batch"):
            t_fwd = timed(forward_only, reps)

        def completion_steps():
            for b in beams:
                SW.completion_sweep(clf, b.view(-1, b.shape[2]), lo, hi, free=1, min_gap=1, top=BEAM, width=width)

        t_comp = timed(completion_steps, reps)
        flags = [torch.zeros(int(x.shape[0]), dtype=torch.int32, device="cuda") for x in xs]

        def kernels_only():
            for b, f in zip(beams, flags):
                twin = SW.grow_twins(b)
                for g0 in range(0, int(f.numel()), chunk):
                    SW.grow_twin_flags(twin, lo, n, f[g0:g0 + chunk], g0, min(chunk, int(f.numel()) - g0))

        t_kern = timed(kernels_only, reps)
        del xs, flags
        torch.cuda.empty_cache()
        print(f"| ({name}) {A} seeds of {s}, beam {BEAM}, max_size {max_size}, width {width} | {out['steps']} | {rows} | {t_grow:.2f} ms | {t_fwd:.2f} ms | "
              f"{t_comp:.2f} ms | {t_kern:.3f} ms | {t_grow / t_fwd:.3f} | {t_grow / t_comp:.3f} | {t_kern / t_fwd:.4f} |", flush=True)
        print(f"  ({name}) candidates {out['n_candidates']}, invalid {out['n_invalid']}, twins {out['n_twins']}, kept {int(out['count'].sum())}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", type=str, default="ab")
    a = ap.parse_args()
    bench(a.reps, [c for c in a.cases if c in CASES])
