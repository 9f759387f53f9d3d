"""Cost of the per-locus scores (matcha_locus_scores: the long-row chain + head_scores_kernel) beside the long forward it is built on, and
the planted-outlier benchmark on a briefly trained model.

  python tools/outlier_bench.py time [--reps 21] [--what both|forward]      one JSON line per width
  MATCHA_HIP_LIB=<a build of the parent commit> python tools/outlier_bench.py time --what forward
  python tools/outlier_bench.py hits [--layout c23] [--sizes 3 4 5] [--epochs2 3]

``time``: d = 64 table model, hg38 at 1 Mb, B = 65 536 full rows at L = 5, 16, 32, the C entries called directly on buffers allocated once
(no torch allocation inside the timed region), device events after a warm-up, the median of --reps; the two entries alternate inside one
process, so both see the same clocks.  ``--what forward`` times matcha_forward_long alone -- the form that runs on a library that does not
have the new entry, i.e. the parent commit's: the comparison DESIGN.md 7.15 quotes is that number against ``scores`` of this build.

``hits``: writes the synthetic k-mer files of the training driver's tests into a scratch directory, trains with matcha_amd.train for a few
epochs, and prints matcha_amd.outlier's report -- hit rates with chance beside them.  The synthetic hyperedges are uniform random sets, so
nothing but memorisation separates a positive's loci from a planted one: the figures say what the pipeline gives, not what a model can do."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, ".")
from matcha_amd import _lib, synth  # noqa: E402
from tools.long_bench import model, rows_of, timed  # noqa: E402


def time_entries(reps, what):
    if what == "forward":              # a library of the parent commit does not export the two new entries: do not ask it for them
        for name in ("matcha_locus_scores", "matcha_outlier_plant"):
            _lib.SIGNATURES.pop(name, None)
    clf, _, num = model()
    N = int(np.sum(num))
    rt = clf._runtime()
    lib = rt.lib
    has_scores = hasattr(lib, "matcha_locus_scores") and what == "both"
    B = 1 << 16
    with torch.no_grad():
        opts, _ = clf._opts(rt, False)
    opts.training, opts.forward_only, opts.status = 0, 1, rt.status.data_ptr()
    for L in (5, 16, 32):
        rng = np.random.default_rng(2027 + L)
        x = torch.from_numpy(np.concatenate([rows_of(rng, N, np.full(1 << 14, L), L) for _ in range(4)])).cuda()
        ws = rt.workspace(B, L, long_rows=True)
        logits = torch.empty(B, dtype=torch.float32, device="cuda")
        scores = torch.empty(B, L, dtype=torch.float32, device="cuda")
        order = torch.empty(B, 3, dtype=torch.long, device="cuda")
        losses = torch.zeros(3, dtype=torch.float32, device="cuda")
        args = (C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L)

        def forward():
            _lib.check(lib.matcha_forward_long(*args, _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream()), "matcha_forward_long")

        def scores_fn():
            _lib.check(lib.matcha_locus_scores(*args, _lib.ptr(scores), _lib.ptr(logits), 3, _lib.ptr(order), _lib.ptr(losses), _lib.ptr(ws), ws.numel(),
                                               rt.stream()), "matcha_locus_scores")

        out = {"B": B, "L": L, "d": 64, "reps": reps, "lib": "MATCHA_HIP_LIB" if os.environ.get("MATCHA_HIP_LIB") else "tree"}
        # alternate the two entries: three rounds of medians, the median of those
        fwd, sco = [], []
        for _ in range(3):
            fwd.append(timed(forward, reps))
            if has_scores:
                sco.append(timed(scores_fn, reps))
        out["forward_long_ms"] = round(float(np.median(fwd)), 4)
        out["forward_long_rounds_ms"] = [round(v, 4) for v in fwd]
        if has_scores:
            out["locus_scores_ms"] = round(float(np.median(sco)), 4)
            out["locus_scores_rounds_ms"] = [round(v, 4) for v in sco]
            out["scores_over_forward"] = round(out["locus_scores_ms"] / out["forward_long_ms"], 4)
            out["extra_store_bytes"] = 4 * B * L + 8 * B * 3
        print(json.dumps(out), flush=True)


def planted_hits(layout, sizes, epochs1, epochs2, batches, top, draws):
    from matcha_amd import outlier as OL, train as T
    import Modules  # noqa: F401
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        temp = os.path.join(tmp, "Temp")
        os.makedirs(temp)
        np.save(os.path.join(temp, "chrom_range.npy"), synth.chrom_range(num))
        n2c = synth.node2chrom(num)
        np.save(os.path.join(temp, "node2chrom.npy"), {int(i): int(n2c[i]) for i in range(1, N + 1)}, allow_pickle=True)
        for k in sorted(set(sizes) | {2}):
            np.save(os.path.join(temp, "all_%d_counter.npy" % k), synth.make_edges(rng, N, k, 4000))
            np.save(os.path.join(temp, "all_%d_freq_counter.npy" % k), synth.make_freq(rng, 4000))
        intra, inter = synth.make_adjacency(rng, num)
        np.save(os.path.join(temp, "intra_adj.npy"), intra)
        np.save(os.path.join(temp, "inter_adj.npy"), inter)
        cfg = {"cluster_path": "x", "mcool_path": "x", "resolution": 1000000, "chrom_list": ["chr%d" % (i + 1) for i in range(len(num))],
               "chrom_size": "x", "temp_dir": temp, "max_cluster_size": 25, "min_distance": 0, "k-mer_size": sorted(sizes), "min_freq_cutoff": 2,
               "quantile_cutoff_for_positive": 0.6, "quantile_cutoff_for_unlabel": 0.4, "embed_dim": 64}
        np.random.seed(0)
        torch.manual_seed(0)
        logs = []
        T.run(cfg, front_end="table", epochs1=epochs1, epochs2=epochs2, batches_per_epoch=batches, emb_path=os.path.join(tmp, "embeddings.npy"), log=logs.append)
        print([l for l in logs if "Validation" in l][-1])
        OL.run(cfg, os.path.join(temp, "model2load"), sizes, top=top, draws=draws)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=21)
    t.add_argument("--what", choices=["both", "forward"], default="both")
    h = sub.add_parser("hits")
    h.add_argument("--layout", default="c23")
    h.add_argument("--sizes", type=int, nargs="+", default=[3, 4, 5])
    h.add_argument("--epochs1", type=int, default=1)
    h.add_argument("--epochs2", type=int, default=3)
    h.add_argument("--batches-per-epoch", type=int, default=40)
    h.add_argument("--top", type=int, default=3)
    h.add_argument("--draws", type=int, default=1)
    a = ap.parse_args()
    if a.cmd == "time":
        time_entries(a.reps, a.what)
    else:
        planted_hits(a.layout, a.sizes, a.epochs1, a.epochs2, a.batches_per_epoch, a.top, a.draws)
