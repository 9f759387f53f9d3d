"""Measure the cluster file's parse: MB/s of ``process.parse_clusters_device`` and of the host ``parse_clusters`` on one file.

    python tools/cluster_parse_bench.py [--mb 256] [--chunk-mb 256] [--repeat 3] [--out profiles/cluster_parse.md]

The file is synthetic, with a size distribution like a SPRITE ``.clusters`` file's: most lines hold 2 .. 10 items, a heavy tail (a Pareto draw)
reaches the pre-filter's 1 250 items, and 0.2 % of the lines lie over the pre-filter of 50 max_cluster_size items; 5 % of the items name a
chromosome that is not listed; terminators are ``\\n``.  The genome is the hg38 layout at 1 Mb (23 chromosomes, 3 067 + 23 bins), max_cluster_size 25.

``device_seconds`` is the whole ``parse_clusters_device(path)``; it is split, each part measured on its own between device synchronisations:
``read_seconds`` (the host's chunk reader alone: file -> buffer, the cut with rfind), ``copy_seconds`` (the chunks' host-to-device copies from
pageable memory) and ``kernel_seconds`` (matcha_cluster_text_count + matcha_cluster_text_parse on device-resident chunks, the sizing read-back
between them included, allocations excluded).  ``host_seconds`` is ``parse_clusters`` on the same file, once.  Medians of ``--repeat`` runs after
one warm-up; the two parsers' results are compared for equality.  Prints one JSON line and writes the table to ``--out``.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matcha_amd import _lib, process as PC, synth  # noqa: E402

RES, MAX_CLUSTER = 1000000, 25


def genome():
    bins = [int(b) for b in synth.LAYOUTS["hg38_1mb"]]
    names = ["chr%d" % (i + 1) for i in range(len(bins) - 1)] + ["chrX"]
    return names, {n: b * RES for n, b in zip(names, bins)}                   # build_node_dict makes ceil(size / res) + 1 bins of each


def write_file(path, target_bytes, seed=11):
    """-> (lines, items, lines over the pre-filter)."""
    rng = np.random.default_rng(seed)
    names, sizes = genome()
    pool = names + ["chrM", "chrUn_KI270742v1"]
    weights = np.asarray([sizes.get(n, 0) for n in pool], dtype=np.float64)
    weights[len(names):] = weights[:len(names)].sum() * 0.025                  # 5 % of the items are on unlisted chromosomes
    weights /= weights.sum()
    tops = np.asarray([sizes.get(n, 16569) for n in pool], dtype=np.int64)
    enc = [n.encode() for n in pool]
    written = lines = items = over = 0
    with open(path, "wb") as f:
        while written < target_bytes:
            batch = 20000
            small = rng.integers(2, 11, size=batch)
            tail = np.minimum((rng.pareto(1.1, size=batch) * 8).astype(np.int64) + 2, 50 * MAX_CLUSTER)
            n_items = np.where(rng.random(batch) < 0.8, small, tail)
            n_items[rng.random(batch) < 0.002] = 50 * MAX_CLUSTER + int(rng.integers(1, 500))
            total = int(n_items.sum())
            chrom = rng.choice(len(pool), size=total, p=weights)
            pos = (rng.random(total) * tops[chrom]).astype(np.int64)
            text = [b"%s:%d" % (enc[c], p) for c, p in zip(chrom.tolist(), pos.tolist())]
            out, at = [], 0
            for k, n in enumerate(n_items.tolist()):
                out.append(b"DPM6G%d.NYBot%d\t" % (lines + k, n) + b"\t".join(text[at:at + n]) + b"\n")
                at += n
            blob = b"".join(out)
            f.write(blob)
            written += len(blob)
            lines += batch
            items += total
            over += int((n_items > 50 * MAX_CLUSTER).sum())
    return lines, items, over


def median_time(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def kernels_on_resident_chunks(chunks_d, table, n_nodes):
    """The two entries on chunks that are already on the device; returns the seconds between synchronisations, allocations excluded."""
    lib = _lib.load()
    dev = chunks_d[0].device
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    names, first, bins = table
    u8 = dict(dtype=torch.uint8, device=dev)
    count_ws = torch.empty(lib.matcha_cluster_text_count_workspace_bytes(0), **u8)
    counts, n_out = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    status = torch.empty(8, dtype=torch.int32, device=dev)
    seconds, largest = 0.0, 0
    for text in chunks_d:
        n = text.numel()
        torch.cuda.synchronize()
        t = time.perf_counter()
        _lib.check(lib.matcha_cluster_text_count(_lib.ptr(text), n, _lib.ptr(counts), _lib.ptr(count_ws), count_ws.numel(), st), "count")
        n_lines, n_tabs = (int(v) for v in counts.tolist())
        seconds += time.perf_counter() - t
        ws_bytes = lib.matcha_cluster_text_workspace_bytes(n, n_lines, n_tabs)
        largest = max(largest, ws_bytes)
        ws = torch.empty(ws_bytes, **u8)
        ids, offsets = torch.empty(max(n_tabs, 1), dtype=torch.int32, device=dev), torch.empty(n_lines + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        _lib.check(lib.matcha_cluster_text_parse(_lib.ptr(text), n, n_lines, n_tabs, names.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p),
                                                 bins.ctypes.data_as(C.c_void_p), len(first), RES, MAX_CLUSTER, n_nodes, _lib.ptr(ids), ids.numel(),
                                                 _lib.ptr(offsets), offsets.numel(), _lib.ptr(n_out), C.c_void_p(n_out.data_ptr() + 8), _lib.ptr(status),
                                                 _lib.ptr(ws), ws_bytes, st), "parse")
        assert status.tolist()[0] == 0
        seconds += time.perf_counter() - t
        del ws, ids, offsets
    return seconds, largest


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mb", type=int, default=256, help="size of the synthetic file")
    ap.add_argument("--chunk-mb", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cluster_parse.md"))
    a = ap.parse_args()
    names, sizes = genome()
    chunk = a.chunk_mb << 20
    with tempfile.TemporaryDirectory() as tmp:
        size_path, path = os.path.join(tmp, "sizes.txt"), os.path.join(tmp, "synthetic.clusters")
        with open(size_path, "w") as f:
            f.write("".join("%s\t%d\n" % (n, sizes[n]) for n in names))
        bin2node, _, _, chrom_range = PC.build_node_dict(size_path, names, RES)
        lines, items, over = write_file(path, a.mb << 20)
        n_bytes = os.path.getsize(path)
        table = PC.cluster_chrom_table(names, chrom_range, RES)
        run = lambda: PC.parse_clusters_device(path, names, chrom_range, RES, MAX_CLUSTER, chunk_bytes=chunk)
        t_device = median_time(run, a.repeat)
        t_read = median_time(lambda: sum(c[2] for c in PC._text_chunks(path, chunk)), a.repeat)
        host_chunks = [bytes(buf[:length]) for _, buf, length in PC._text_chunks(path, chunk)]
        host_chunks = [bytearray(c) for c in host_chunks]                     # writable, as the reader's buffer is
        t_copy = median_time(lambda: [torch.frombuffer(c, dtype=torch.uint8).to("cuda") for c in host_chunks], a.repeat)
        chunks_d = [torch.frombuffer(c, dtype=torch.uint8).to("cuda") for c in host_chunks]
        del host_chunks
        kernels_on_resident_chunks(chunks_d, table[:3], table[3])
        runs = [kernels_on_resident_chunks(chunks_d, table[:3], table[3]) for _ in range(a.repeat)]
        t_kernel, ws_bytes = float(np.median([r[0] for r in runs])), runs[0][1]
        del chunks_d
        ids_d, off_d = run()
        t = time.perf_counter()
        clusters = PC.parse_clusters(path, bin2node, names, RES, MAX_CLUSTER)
        t_host = time.perf_counter() - t
    ids, off = ids_d.cpu().numpy(), off_d.cpu().numpy()
    assert len(clusters) == len(off) - 1 and np.array_equal(np.diff(off), [len(c) for c in clusters])
    assert np.array_equal(ids, np.fromiter((v for c in clusters for v in c), dtype=np.int32, count=len(ids)))
    mb = n_bytes / 1e6
    res = dict(what="cluster_parse", bytes=n_bytes, lines=lines, items=items, lines_over_prefilter=over, clusters=len(clusters), ids=int(len(ids)),
               chunk_bytes=chunk, chunks=-(-n_bytes // chunk), device_seconds=t_device, read_seconds=t_read, copy_seconds=t_copy,
               kernel_seconds=t_kernel, host_seconds=t_host, device_mb_per_s=mb / t_device, kernel_mb_per_s=mb / t_kernel,
               kernel_items_per_s=items / t_kernel, host_mb_per_s=mb / t_host, speedup=t_host / t_device, largest_workspace_bytes=int(ws_bytes))
    print(json.dumps(res))
    rows = [("file", "%.1f MB, %d lines, %d items (%d lines over the pre-filter), %d kept clusters with %d ids" % (mb, lines, items, over, len(clusters), len(ids))),
            ("`parse_clusters_device`, whole", "%.1f ms, %.0f MB/s" % (1e3 * t_device, mb / t_device)),
            ("... the chunk reader alone", "%.1f ms, %.0f MB/s" % (1e3 * t_read, mb / t_read)),
            ("... the host-to-device copies alone", "%.1f ms, %.0f MB/s" % (1e3 * t_copy, mb / t_copy)),
            ("... the two entries on resident chunks", "%.1f ms, %.0f MB/s, %.0f M items/s" % (1e3 * t_kernel, mb / t_kernel, items / t_kernel / 1e6)),
            ("`parse_clusters` (host), once", "%.2f s, %.1f MB/s" % (t_host, mb / t_host)),
            ("device over host, whole", "%.0fx" % (t_host / t_device)),
            ("largest chunk workspace", "%.0f MB" % (ws_bytes / 1e6))]
    with open(a.out, "w") as f:
        f.write("# The cluster file's parse (DESIGN.md §7.19): what it costs\n\n")
        f.write("`python tools/cluster_parse_bench.py --mb %d --chunk-mb %d --repeat %d` on one MI355X; a synthetic file (most lines 2-10 items, a Pareto\n"
                "tail to 1 250, 0.2 %% of the lines over the pre-filter, 5 %% of the items on unlisted chromosomes), hg38 at 1 Mb, max_cluster_size %d.\n"
                "Host clock between device synchronisations, one warm-up, medians of %d; the file is in the page cache.  The two parsers' clusters are\n"
                "compared for equality in the same run.\n\n" % (a.mb, a.chunk_mb, a.repeat, MAX_CLUSTER, a.repeat))
        f.write("| what | measured |\n|---|---|\n" + "".join("| %s | %s |\n" % r for r in rows))
    return res


if __name__ == "__main__":
    main()
