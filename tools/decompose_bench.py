"""Cost of cluster decomposition (matcha_amd/sweep.py::decomposition_sweep, cluster_subset_rows_kernel and subset_support_update_kernel;
DESIGN.md 7.11) beside the eval forward on the same rows.

  python tools/decompose_bench.py [--reps 10] [--cases abc] [--pairs]

d = 64 table model, hg38 at 1 Mb, eval mode under no_grad, timed with device events after a warm-up (median of --reps), one process per
case, as tools/complete_bench.py.  Cluster ids are drawn from the whole genome, min_gap 1, top 20:

  (a) 2 000 clusters of s uniform in [9, 25] ids, keep m = 3 (width 3: the L <= 8 forward),
  (b) 2 000 clusters of s uniform in [9, 25] ids, drop m = 1, width 25 (the long forward),
  (c) 200 clusters of 32 ids, keep m = 4 (width 4),

and per case, in the same run: the sweep; the yardstick, model(x) alone over the same candidate rows, generated beforehand, in the
sweep's groups and chunks and on its route; the rows kernel alone over all ranks in the same chunks; the support kernel alone over the
same chunks with values and skip flags made beforehand.  --pairs appends, from the same run: the pair kernel
(subset_pair_update_kernel) alone over the same chunks, values and flags; the sweep with pair_support=True; their ratios to model(x), to
the unchanged support kernel and to the sweep without.  Case (b) drops one locus, which has no pair: its pair columns read n/a."""
import argparse
import math
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import _lib  # noqa: E402
from matcha_amd import sweep as SW  # noqa: E402
from tools.long_bench import model, timed  # noqa: E402

CASES = {"a": (2000, (9, 25), 3, "keep", None), "b": (2000, (9, 25), 1, "drop", 25), "c": (200, (32, 32), 4, "keep", None)}   # clusters, sizes, m, mode, width


def clusters_of(rng, N, A, sizes):
    t = np.zeros((A, sizes[1]), dtype=np.int64)
    for a, s in enumerate(rng.integers(sizes[0], sizes[1] + 1, size=A)):
        t[a, :s] = np.sort(rng.choice(N, size=int(s), replace=False) + 1)
    return t


def bench(reps, which, pairs=False):
    clf, _, num = model()
    N = int(np.sum(num))
    rng = np.random.default_rng(2028)
    print("| case | rows | groups | chunk | sweep | model(x) on the same rows | rows kernel alone | support kernel alone | sweep / model(x) | rows kernel / model(x) | "
          "support kernel / model(x) |" + (" pair kernel alone | sweep with pairs | pair kernel / model(x) | pair kernel / support kernel | "
                                           "sweep with pairs / sweep |" if pairs else ""))
    print("|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|---|---|---|" if pairs else ""))
    for name in which:
        A, sizes, m, mode, width = CASES[name]
        comp = int(mode == "drop")
        table, s_max = SW._subset_table(clusters_of(rng, N, A, sizes), "cuda")
        width = (m if not comp else s_max) if width is None else width
        chunk_rows = 1 << 20 if width <= 8 else min(1 << 20, (1 << 21) // width)
        size = (table != 0).sum(dim=1)
        groups = []                                                      # the sweep's own grouping: (table [A_s, s], C(s, m), chunk)
        for s in sorted(set(size.tolist())):
            tab = table[size == s][:, :s].contiguous()
            groups.append((tab, math.comb(s, m), min(chunk_rows, tab.shape[0] * math.comb(s, m))))
        total = sum(tab.shape[0] * cm for tab, cm, _ in groups)
        t_sweep = timed(lambda: SW.decomposition_sweep(clf, table, m, mode=mode, min_gap=1, top=20, width=width), reps)
        most = max(chunk for _, _, chunk in groups)
        buf = torch.empty(most * width, dtype=torch.long, device="cuda")
        fbuf = torch.empty(most, dtype=torch.int32, device="cuda")

        def rows_only():
            for tab, cm, chunk in groups:
                for g0 in range(0, tab.shape[0] * cm, chunk):
                    SW._subset_rows(tab, m, comp, 1, g0, min(chunk, tab.shape[0] * cm - g0), None, width, buf, fbuf)

        t_rows = timed(rows_only, reps)
        xs = [SW._subset_rows(tab, m, comp, 1, 0, None, None, width, None, None) for tab, _, _ in groups]
        vals = [torch.rand(x.shape[0], device="cuda") for x, _ in xs]
        sups = [SW.SubsetSupport(tab.shape[0], tab.shape[1], m, device="cuda") for tab, _, _ in groups]

        def support_only():
            for (tab, cm, chunk), (_, flag), v, sup in zip(groups, xs, vals, sups):
                for g0 in range(0, tab.shape[0] * cm, chunk):
                    sup.update(v[g0:g0 + chunk], g0, flag[g0:g0 + chunk])

        t_sup = timed(support_only, reps)
        t_pair = t_both = None
        if pairs and m >= 2:
            psups = [SW.SubsetPairSupport(tab.shape[0], tab.shape[1], m, device="cuda") for tab, _, _ in groups]

            def pairs_only():
                for (tab, cm, chunk), (_, flag), v, sup in zip(groups, xs, vals, psups):
                    for g0 in range(0, tab.shape[0] * cm, chunk):
                        sup.update(v[g0:g0 + chunk], g0, flag[g0:g0 + chunk])

            t_pair = timed(pairs_only, reps)
            del psups
            t_both = timed(lambda: SW.decomposition_sweep(clf, table, m, mode=mode, min_gap=1, top=20, width=width, pair_support=True), reps)

        def forward_only():
            for (tab, cm, chunk), (x, _) in zip(groups, xs):
                for g0 in range(0, x.shape[0], chunk):
                    clf(x[g0:g0 + chunk])

        with torch.no_grad(), clf.deferred_id_check(), _lib.option("disable_small_batch"):
            t_fwd = timed(forward_only, reps)
        del xs, vals, sups, buf, fbuf
        torch.cuda.empty_cache()
        print(f"| ({name}) {A} clusters of {sizes[0]}..{sizes[1]}, {mode} m = {m}, width {width} | {total} | {len(groups)} | {most} | {t_sweep:.2f} ms | "
              f"{t_fwd:.2f} ms | {t_rows:.3f} ms | {t_sup:.3f} ms | {t_sweep / t_fwd:.3f} | {t_rows / t_fwd:.4f} | {t_sup / t_fwd:.4f} |"
              + ((f" {t_pair:.3f} ms | {t_both:.2f} ms | {t_pair / t_fwd:.4f} | {t_pair / t_sup:.2f} | {t_both / t_sweep:.3f} |" if t_pair is not None
                  else " n/a | n/a | n/a | n/a | n/a |") if pairs else ""), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", type=str, default="abc")
    ap.add_argument("--pairs", action="store_true", help="also time the pair kernel alone and the sweep with pair_support=True")
    a = ap.parse_args()
    bench(a.reps, [c for c in a.cases if c in CASES], a.pairs)
