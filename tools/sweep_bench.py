"""Cost of the de novo k-way sweep (csrc/sweep_rows.hip, csrc/sweep_select.hip, matcha_amd/sweep.py) beside the forward it feeds.

  python tools/sweep_bench.py [--top 10000] [--chunk-rows 1048576] [--sweep-only] [--stats kernel_stats.csv]
  python tools/sweep_bench.py --anchored [--chunk-rows 1048576] [--sweep-only]
  python tools/sweep_bench.py --map [--chunk-rows 1048576] [--sweep-only]

d = 64 table model, hg38 at 1 Mb, chr1 (250 bins), min_gap 1: k = 3 over the whole chromosome (2 573 000 candidates) and k = 4 over
its first 2^26 ranks, timed end to end with device events after a warm-up (candidates/s); then, on one steady-state chunk of k = 4
(the selection already holds ``top`` pairs), kway_rows, the forward and the TopK update each on their own, so the two new stages
stand next to the forward of the same chunk in the same run.  By bytes kway_rows writes 8 k bytes per row and the update reads 4
(the radix sort of the chunk's 32-bit keys and indices is on top: four passes over 8 bytes per row, read and written).
--sweep-only runs the k = 4 sweep alone (the run to put under rocprofv3 --kernel-trace --stats); --stats reads that run's
kernel_stats.csv and prints the share of kway_rows_kernel, of the selection (select_*, *topk_keys and the radix sort) and of everything else (the
forward).
--anchored: the anchored sweep at k = 3 with every bin of chr1 an anchor and chr1 as partner region (250 x 31 125
global ranks), top 100 per anchor, beside the plain k = 3 kway_sweep (top 100) in the same run, rows/s by device events after a
warm-up; with --sweep-only the anchored sweep alone (the run to put under rocprofv3 --kernel-trace --stats).
--map: kway_map over the whole of chr1 at k = 3 and k = 4 (all four planes) beside kway_sweep (top ``--top``) on the
same region in the same run, by device events after a warm-up; then, on one chunk of each k, the forward and PairMap.update (all
planes, and the sum alone) each on their own.  With --sweep-only the k = 3 map alone, three times (the run to put under rocprofv3
--kernel-trace --stats; --stats then also lists the share of pairmap_*)."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import sweep as SW
from matcha_amd import synth

K4_RANKS = 1 << 26


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


def sweep_ranks(clf, lo, n, k, min_gap, top, chunk_rows, n_ranks):
    """kway_sweep's loop over the first ``n_ranks`` ranks only (the public pieces, in its order)."""
    sel = SW.TopK(top, chunk_rows, "cuda")
    buf = torch.empty(chunk_rows * k, dtype=torch.long, device="cuda")
    with torch.no_grad(), clf.deferred_id_check():
        for r0 in range(0, n_ranks, chunk_rows):
            x = SW.kway_rows(lo, n, k, min_gap, rank0=r0, count=min(chunk_rows, n_ranks - r0), out=buf)
            sel.update(clf(x).reshape(-1), r0)
    logit, rank = sel.result()
    return SW.kway_rows(lo, n, k, min_gap, ranks=rank), logit


def model():
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    clf, _ = hip_model(num, 64, "table", 12)
    clf.eval()
    cr = np.asarray(synth.chrom_range(num))
    return clf, int(cr[0][0]), int(cr[0][1])


def bench(top, chunk_rows, sweep_only):
    clf, lo, hi = model()
    n = hi - lo
    if sweep_only:
        sweep_ranks(clf, lo, n, 4, 1, top, chunk_rows, K4_RANKS)
        torch.cuda.synchronize()
        return
    total3 = SW.kway_count(n, 3, 1)
    t3 = timed(lambda: SW.kway_sweep(clf, lo, hi, 3, 1, top, chunk_rows=chunk_rows), 3)
    print(f"k=3 whole chromosome: {total3} candidates, top {top}, chunk {chunk_rows}: {t3:.1f} ms end to end, {total3 / t3 / 1e3:.1f} M candidates/s", flush=True)
    t4 = timed(lambda: sweep_ranks(clf, lo, n, 4, 1, top, chunk_rows, K4_RANKS), 2)
    print(f"k=4 first 2^26 ranks of {SW.kway_count(n, 4, 1)}: {t4:.1f} ms end to end, {K4_RANKS / t4 / 1e3:.1f} M candidates/s", flush=True)
    # one steady-state chunk: the stages on their own
    for k in (3, 4):
        rows = min(chunk_rows, SW.kway_count(n, k, 1))
        buf = torch.empty(rows * k, dtype=torch.long, device="cuda")
        sel = SW.TopK(top, rows, "cuda")
        with torch.no_grad(), clf.deferred_id_check():
            x = SW.kway_rows(lo, n, k, 1, rank0=0, count=rows, out=buf)
            logits = clf(x).reshape(-1)
            sel.update(logits, 0)                                         # the state is full from here on
            t_rows = timed(lambda: SW.kway_rows(lo, n, k, 1, rank0=rows // 2, count=rows, out=buf) if SW.kway_count(n, k, 1) >= rows + rows // 2
                           else SW.kway_rows(lo, n, k, 1, rank0=0, count=rows, out=buf), 10)
            t_fwd = timed(lambda: clf(x), 10)
            t_upd = timed(lambda: sel.update(logits, rows), 10)
        print(f"k={k} chunk of {rows} rows: kway_rows {t_rows:.3f} ms ({100 * t_rows / t_fwd:.1f} % of the forward; {8 * k * rows / t_rows / 1e6:.0f} GB/s written), "
              f"forward {t_fwd:.3f} ms ({rows / t_fwd / 1e3:.1f} M rows/s), TopK update {t_upd:.3f} ms ({100 * t_upd / t_fwd:.1f} % of the forward)", flush=True)


def bench_anchored(chunk_rows, sweep_only):
    clf, lo, hi = model()
    anchors = torch.arange(lo, hi, device="cuda")
    total = SW.anchored_count(hi - lo, 1, hi - lo, 3, 1)
    run = lambda: SW.anchored_sweep(clf, anchors, lo, hi, 3, 1, 100, chunk_rows=chunk_rows)
    if sweep_only:
        run()
        torch.cuda.synchronize()
        return
    ta = timed(run, 3)
    print(f"anchored k=3, 250 anchors x chr1: {total} global ranks, top 100 per anchor, chunk {chunk_rows}: {ta:.1f} ms end to end, "
          f"{total / ta / 1e3:.1f} M rows/s", flush=True)
    total3 = SW.kway_count(hi - lo, 3, 1)
    t3 = timed(lambda: SW.kway_sweep(clf, lo, hi, 3, 1, 100, chunk_rows=chunk_rows), 3)
    print(f"plain kway_sweep k=3: {total3} candidates, top 100, chunk {chunk_rows}: {t3:.1f} ms end to end, {total3 / t3 / 1e3:.1f} M rows/s", flush=True)


def bench_map(top, chunk_rows, sweep_only):
    clf, lo, hi = model()
    n = hi - lo
    if sweep_only:
        for _ in range(3):
            SW.kway_map(clf, lo, hi, 3, 1, chunk_rows=chunk_rows)
        torch.cuda.synchronize()
        return
    for k, reps in ((3, 5), (4, 1)):
        total = SW.kway_count(n, k, 1)
        tm = timed(lambda: SW.kway_map(clf, lo, hi, k, 1, chunk_rows=chunk_rows), reps)
        ts = timed(lambda: SW.kway_sweep(clf, lo, hi, k, 1, top, chunk_rows=chunk_rows), reps)
        print(f"k={k} chr1: {total} candidates, chunk {chunk_rows}: kway_map {tm:.1f} ms ({total / tm / 1e3:.1f} M candidates/s), "
              f"kway_sweep top {top} {ts:.1f} ms ({total / ts / 1e3:.1f} M candidates/s), map / sweep {tm / ts:.3f}", flush=True)
    for k in (3, 4):
        rows = min(chunk_rows, SW.kway_count(n, k, 1))
        buf = torch.empty(rows * k, dtype=torch.long, device="cuda")
        with torch.no_grad(), clf.deferred_id_check():
            x = SW.kway_rows(lo, n, k, 1, rank0=0, count=rows, out=buf)
            value = torch.sigmoid(clf(x).reshape(-1))
            t_fwd = timed(lambda: clf(x), 10)
            line = f"k={k} chunk of {rows} rows: forward {t_fwd:.3f} ms"
            for planes in ("all", ["sum"]):
                pm = SW.PairMap((lo, n), (lo, n), planes)
                t_upd = timed(lambda: pm.update(x, value), 10)
                cells = rows * k * (k - 1) // 2
                line += f"; PairMap.update {planes} {t_upd:.3f} ms ({100 * t_upd / t_fwd:.1f} % of the forward, {cells / t_upd / 1e6:.2f} G cell updates/s)"
            shuffled = x[torch.randperm(rows, device="cuda")].contiguous()
            pm = SW.PairMap((lo, n), (lo, n), "all")
            t_shuf = timed(lambda: pm.update(shuffled, value), 10)
            line += f"; the same rows shuffled (no runs to merge) {t_shuf:.3f} ms"
        print(line, flush=True)


def stats(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    groups = {"kway_rows_kernel": 0.0, "selection (select_* + radix sort)": 0.0, "pair map (pairmap_*)": 0.0, "everything else (the forward)": 0.0}
    for r in rows:
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "kway_rows_kernel" in name or "kway_anchor_rows_kernel" in name:
            groups["kway_rows_kernel"] += ns
        elif "pairmap_" in name:
            groups["pair map (pairmap_*)"] += ns
        elif "select_" in name or "topk_" in name or "rocprim" in name.lower() or "radix" in name.lower():
            groups["selection (select_* + radix sort)"] += ns
        else:
            groups["everything else (the forward)"] += ns
    total = sum(groups.values())
    print(f"kernel time of the profiled run ({path}): {total / 1e6:.1f} ms")
    for g, ns in groups.items():
        print(f"  {g:34s} {ns / 1e6:9.2f} ms  {100 * ns / total:5.1f} %")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
        print(f"    {float(r['TotalDurationNs']) / 1e6:9.2f} ms  {int(r['Calls']):6d} calls  {r['Name'][:90]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=int, default=10000)
    ap.add_argument("--chunk-rows", type=int, default=1 << 20)
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--stats", type=str, default=None)
    ap.add_argument("--anchored", action="store_true")
    ap.add_argument("--map", action="store_true")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    elif a.map:
        bench_map(a.top, a.chunk_rows, a.sweep_only)
    elif a.anchored:
        bench_anchored(a.chunk_rows, a.sweep_only)
    else:
        bench(a.top, a.chunk_rows, a.sweep_only)
