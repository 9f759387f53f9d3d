"""Cost of the distance-matched expectation (csrc/expected.hip, matcha_amd/expected.py) beside the forward it rides on.

  python tools/expected_bench.py [--chunk-rows 1048576] [--top 10000] [--k4-bins 128]

d = 64 table model, hg38 at 1 Mb, chr1 (250 bins), min_gap 1, default gap edges (2 .. 128: 8 classes).  By device events after a warm-up,
the median of the repetitions:
  per chunk of k = 3 and k = 4 rows: the forward alone; GapStats.update (all three planes) on the block-level (LDS) path and with every add
  sent straight to global memory (direct=True), on the sweep's ordered rows and on the same rows shuffled; gap_enrich; and
  PairMap.update (sum + count planes) on the same rows -- the yardstick: it addresses C(k, 2) cells per row where GapStats addresses one;
  whole sweeps: kway_enriched_sweep with its two forwards (cache_rows=0), with the first pass's logits kept (the default), and kway_sweep on
  the same region -- k = 3 over all of chr1, k = 4 over its first --k4-bins bins (all of chr1 is 159 M candidates per pass)."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import expected as EX
from matcha_amd import sweep as SW
from tools.sweep_bench import model, timed


def chunk_costs(clf, lo, n, k, chunk_rows):
    rows = min(chunk_rows, SW.kway_count(n, k, 1))
    strata = EX.GapStrata(k, EX.default_gap_edges(n, k))
    buf = torch.empty(rows * k, dtype=torch.long, device="cuda")
    with torch.no_grad(), clf.deferred_id_check():
        x = SW.kway_rows(lo, n, k, 1, rank0=0, count=rows, out=buf)
        logits = clf(x).reshape(-1)
        value = torch.sigmoid(logits)
        t_fwd = timed(lambda: clf(x), 10)
    shuffled = x[torch.randperm(rows, device="cuda")].contiguous()
    line = f"k={k} chunk of {rows} rows, {strata.n_strata} strata: forward {t_fwd:.3f} ms"
    for name, direct in (("LDS", False), ("direct", True)):
        st = EX.GapStats(strata, "all", direct=direct)
        t = timed(lambda: st.update(x, value), 20)
        ts = timed(lambda: st.update(shuffled, value), 20)
        line += f"; GapStats.update {name} {t:.4f} ms ({100 * t / t_fwd:.2f} % of the forward), shuffled {ts:.4f} ms"
    ex = EX.GapExpected(k, strata.edges, 1, k, "class", [(lo, lo + n)], np.full(strata.n_strata, 100), np.full(strata.n_strata, 0.5), None, 0, 0)
    offset, scale = ex.table("logodds", 30)
    t_enr = timed(lambda: strata.enrich(x, logits, offset, scale, want_strata=True), 20)
    pm = SW.PairMap((lo, n), (lo, n), ["sum", "count"])
    t_pm = timed(lambda: pm.update(x, value), 20)
    line += f"; gap_enrich {t_enr:.4f} ms ({100 * t_enr / t_fwd:.2f} %); PairMap.update sum+count {t_pm:.4f} ms ({100 * t_pm / t_fwd:.2f} %)"
    print(line, flush=True)


def whole_sweeps(clf, lo, hi, k, top, chunk_rows, reps):
    total = SW.kway_count(hi - lo, k, 1)
    big = 1 << 40
    t_plain = timed(lambda: SW.kway_sweep(clf, lo, hi, k, 1, top, chunk_rows=chunk_rows), reps)
    t_two = timed(lambda: EX.kway_enriched_sweep(clf, lo, hi, k, 1, top, chunk_rows=chunk_rows, cache_rows=0), reps)
    t_cached = timed(lambda: EX.kway_enriched_sweep(clf, lo, hi, k, 1, top, chunk_rows=chunk_rows, cache_rows=big), reps)
    t_exp = timed(lambda: EX.kway_expected(clf, [(lo, hi)], k, 1, chunk_rows=chunk_rows), reps)
    print(f"k={k} bins [{lo}, {hi}): {total} candidates, top {top}, chunk {chunk_rows}: kway_sweep {t_plain:.1f} ms ({total / t_plain / 1e3:.1f} M candidates/s); "
          f"kway_expected alone {t_exp:.1f} ms ({t_exp / t_plain:.3f} x); enriched, two forwards {t_two:.1f} ms ({t_two / t_plain:.3f} x); "
          f"enriched, logits cached {t_cached:.1f} ms ({t_cached / t_plain:.3f} x)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=int, default=10000)
    ap.add_argument("--chunk-rows", type=int, default=1 << 20)
    ap.add_argument("--k4-bins", type=int, default=128)
    a = ap.parse_args()
    clf, lo, hi = model()
    for k in (3, 4):
        chunk_costs(clf, lo, hi - lo, k, a.chunk_rows)
    whole_sweeps(clf, lo, hi, 3, a.top, a.chunk_rows, 3)
    whole_sweeps(clf, lo, lo + a.k4_bins, 4, a.top, a.chunk_rows, 2)
