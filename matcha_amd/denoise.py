"""Denoised contact maps: the reference's ``denoise_contact.py`` (Code/denoise_contact.py:91-236) on the device.

For every chromosome ``[lo, hi)`` of ``chrom_range`` (n = hi - lo bins): the pairwise sweep of the trained classifier
(``predict.pairwise_probabilities``: sigmoid, or softplus for ``task_mode='regress'``), then the post-processing of
:160-207 in ``csrc/denoise.hip`` -- the symmetric probability matrix P and the observed matrix O of ``intra_adj``, their
coverage normalisation, ``my = maximum(my_proba * origin_part, my_proba)`` and its own coverage, the gap rows / columns of O
-- then ``QuantileTransformer(n_quantiles=1000, 'uniform')`` of ``my``, ``origin_part`` (and ``my_proba`` on request) in
``matcha_quantile_uniform``, and the pixels ``balanced = my_q[i - lo, j - lo]`` in pair order.  For the same probabilities
and the same observed block every matrix and every pixel equals the reference's numpy bit for bit, with three deliberate
differences:

  (a) the quantile fit uses all n^2 values (``subsample=None``); scikit-learn's default fits on a random 10 000-value
      sample once n^2 > 10 000 (n > 100), so the results are identical up to n = 100;
  (b) a chromosome without pairs (n <= min_distance) gives no pixels and no matrices; the reference crashes there;
  (c) the cooler datasets always go to an ``.npz`` and to ``.mcool`` only when h5py imports; the matrices the reference
      plots (``<chrom>_denoise.png``, ``<chrom>_origin.png``) are saved as ``.npy``.

CLI:  python -m matcha_amd.denoise [--config ./config.JSON] [--out-dir ..] [--chrom IDX ...] [--task-mode class|regress]
                                   [--no-matrices]
(reads config.JSON like the reference: temp_dir, resolution, chrom_list, min_distance; and temp_dir/{model2load,
chrom_range.npy, node2bin.npy, intra_adj.npy}, the last one memory-mapped: only each chromosome's block is copied.)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .predict import pairwise_probabilities

N_QUANTILES = 1000          # denoise_contact.py:105


def pair_count(n: int, min_dis: int) -> int:
    """Number of pairs (i, j), i + min_dis <= j, of a chromosome of n bins (denoise_contact.py:67-74)."""
    k = max(0, int(n) - int(min_dis))
    return k * (k + 1) // 2


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _quantile(x: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty_like(x)
    _lib.check(lib.matcha_quantile_uniform(_lib.ptr(x), x.numel(), N_QUANTILES, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(),
                                           _stream(x.device)), "matcha_quantile_uniform")
    return out


def denoise_from_proba(proba, origin_block, n: int, min_dis: int, quantile_proba: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """The post-processing of one chromosome (denoise_contact.py:160-207) on the device.

    proba         float32 [pair_count(n, min_dis)]: the sweep's probabilities in generate_pair_wise order
    origin_block  float32 [n, n] (a view with unit column stride is fine): intra_adj[lo-1:hi-1, lo-1:hi-1]
    Returns device tensors: ``my``, ``origin_part``, ``my_proba`` (the matrices handed to the quantile transforms, my and my_proba
    with the gaps zeroed), ``gap1`` / ``gap2`` (bool [n]: rows / columns of O summing to 0), ``my_q`` and ``origin_q`` (the
    transformed matrices), ``my_proba_q`` (only with ``quantile_proba``; the reference computes it and writes it nowhere) and
    ``balanced`` (float32 [n_pairs]).  With no pairs (n <= min_dis) every entry is empty and nothing is launched."""
    n, min_dis = int(n), int(min_dis)
    if min_dis < 0:
        raise ValueError("min_dis must be >= 0")
    n_pairs = pair_count(n, min_dis)
    dev = proba.device if isinstance(proba, torch.Tensor) else torch.device("cuda")
    if n_pairs == 0:
        z2 = torch.empty(0, 0, dtype=torch.float32, device=dev)
        zb = torch.empty(0, dtype=torch.bool, device=dev)
        return {"my": z2, "origin_part": z2, "my_proba": z2, "gap1": zb, "gap2": zb, "my_q": z2, "origin_q": z2,
                "my_proba_q": z2 if quantile_proba else None, "balanced": torch.empty(0, dtype=torch.float32, device=dev)}
    p = torch.as_tensor(proba, dtype=torch.float32, device=dev).contiguous()
    o = torch.as_tensor(origin_block, dtype=torch.float32, device=dev)
    if o.dim() != 2 or o.shape[0] < n or o.shape[1] < n:
        raise ValueError("origin_block must be a [n, n] matrix (or a larger one whose top-left n x n block is used)")
    if o.stride(1) != 1:
        o = o[:n, :n].contiguous()
    lib = _lib.load()
    my = torch.empty(n, n, dtype=torch.float32, device=dev)
    origin_part = torch.empty_like(my)
    my_proba = torch.empty_like(my)
    gap = torch.empty(2 * n, dtype=torch.uint8, device=dev)
    ws_bytes = lib.matcha_denoise_workspace_bytes(n)
    if ws_bytes == 0:
        raise _lib.MatchaHipError("matcha_denoise_workspace_bytes: n out of range (n * n must stay below 2^31)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = _stream(dev)
    _lib.check(lib.matcha_denoise_intra(_lib.ptr(p), p.numel(), n, min_dis, _lib.ptr(o), o.stride(0), _lib.ptr(my),
                                        _lib.ptr(origin_part), _lib.ptr(my_proba), _lib.ptr(gap), _lib.ptr(ws), ws_bytes, st),
               "matcha_denoise_intra")
    qws = torch.empty(lib.matcha_quantile_workspace_bytes(n * n), dtype=torch.uint8, device=dev)
    my_q = _quantile(my, qws)                       # :190-192, in the reference's order
    origin_q = _quantile(origin_part, qws)
    my_proba_q = _quantile(my_proba, qws) if quantile_proba else None
    balanced = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    _lib.check(lib.matcha_denoise_pixels(_lib.ptr(my_q), n, min_dis, _lib.ptr(balanced), st), "matcha_denoise_pixels")
    return {"my": my, "origin_part": origin_part, "my_proba": my_proba, "gap1": gap[:n].bool(), "gap2": gap[n:].bool(),
            "my_q": my_q, "origin_q": origin_q, "my_proba_q": my_proba_q, "balanced": balanced}


def denoise_chromosome(model, chrom_range, chrom_id: int, min_dis: int, origin_block, task_mode: str = "class",
                       quantile_proba: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """denoise_contact.py:148-207 for one chromosome: the device sweep (``pairwise_probabilities``), then ``denoise_from_proba``.
    Adds ``proba`` (float32 [n_pairs]) and ``pairs`` (int64 [n_pairs, 2] node ids) to the result."""
    lo, hi = int(chrom_range[chrom_id][0]), int(chrom_range[chrom_id][1])
    pairs, proba = pairwise_probabilities(model, chrom_range, chrom_id, min_dis, task_mode=task_mode)
    out = denoise_from_proba(proba, origin_block, hi - lo, min_dis, quantile_proba)
    out["proba"], out["pairs"] = proba, pairs
    return out


def cooler_tables(node2bin: Dict[int, str], chrom_names: Sequence[str], res: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[str]]:
    """(chrom index, start, end) of every node id 1 .. max id, and the chromosome names (denoise_contact.py:120-139)."""
    chrom, start, end = [], [], []
    for i in range(1, int(np.max(list(node2bin.keys()))) + 1):
        c, s = node2bin[i].split(":")
        chrom.append(list(chrom_names).index(c))
        start.append(int(s))
        end.append(int(s) + int(res))
    return np.asarray(chrom, dtype=np.int64), np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64), list(chrom_names)


def _write_mcool(path: str, datasets: Dict[str, np.ndarray]) -> bool:
    """The reference's .mcool layout (:114-140, :234-236), when h5py is importable."""
    try:
        import h5py
    except ImportError:
        return False
    with h5py.File(path, "w") as f:
        for key, data in datasets.items():
            if key.endswith("chroms/name"):
                f.create_dataset(key, data=[s.encode("utf8") for s in data], dtype=h5py.special_dtype(vlen=str))
            else:
                f.create_dataset(key, data=data)
    return True


def main(argv=None):
    ap = argparse.ArgumentParser(description="denoise_contact.py on the MI355X path: denoised intra-chromosomal contact maps")
    ap.add_argument("--config", type=str, default="./config.JSON")
    ap.add_argument("--out-dir", type=str, default="..", help="where denoised_pixels.npz, denoised.mcool and the matrices go "
                                                                "(the reference writes to ..)")
    ap.add_argument("--chrom", type=int, nargs="*", default=None, help="indices into config chrom_list (default: all)")
    ap.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's objective: sigmoid or softplus")
    ap.add_argument("--no-matrices", action="store_true", help="skip <chrom>_denoise.npy / <chrom>_origin.npy")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    temp_dir, res, names, min_dis = config["temp_dir"], int(config["resolution"]), list(config["chrom_list"]), int(config["min_distance"])
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    model = torch.load(os.path.join(temp_dir, "model2load"), map_location="cuda", weights_only=False)
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    origin = np.load(os.path.join(temp_dir, "intra_adj.npy"), mmap_mode="r")
    os.makedirs(args.out_dir, exist_ok=True)
    chrom_ids = args.chrom if args.chrom else list(range(len(names)))
    bin1, bin2, balanced = [], [], []
    for cid in chrom_ids:
        lo, hi = int(chrom_range[cid][0]), int(chrom_range[cid][1])
        block = torch.from_numpy(np.ascontiguousarray(origin[lo - 1:hi - 1, lo - 1:hi - 1], dtype=np.float32)).cuda()
        out = denoise_chromosome(model, chrom_range, cid, min_dis, block, task_mode=args.task_mode)
        if out["balanced"].numel() == 0:
            print("%s: no pairs at min_distance %d, skipped" % (names[cid], min_dis))
            continue
        ids = out["pairs"] - 1
        bin1.append(ids[:, 0].cpu().numpy())
        bin2.append(ids[:, 1].cpu().numpy())
        balanced.append(out["balanced"].cpu().numpy())
        if not args.no_matrices:
            np.save(os.path.join(args.out_dir, "%s_denoise.npy" % names[cid]), out["my_q"].cpu().numpy())
            np.save(os.path.join(args.out_dir, "%s_origin.npy" % names[cid]), out["origin_q"].cpu().numpy())
        print("%s: %d bins, %d pixels" % (names[cid], hi - lo, out["balanced"].numel()))
    chrom, start, end, chrom_names = cooler_tables(node2bin, names, res)
    g = "resolutions/%d/" % res
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    datasets = {g + "bins/chrom": chrom, g + "bins/start": start, g + "bins/end": end, g + "chroms/name": np.array(chrom_names),
                g + "pixels/bin1_id": cat(bin1, np.int64), g + "pixels/bin2_id": cat(bin2, np.int64),
                g + "pixels/balanced": cat(balanced, np.float32)}
    np.savez(os.path.join(args.out_dir, "denoised_pixels.npz"), **datasets)
    wrote = _write_mcool(os.path.join(args.out_dir, "denoised.mcool"), datasets)
    print("%d pixels -> %s%s" % (len(datasets[g + "pixels/balanced"]), os.path.join(args.out_dir, "denoised_pixels.npz"),
                                  " and denoised.mcool" if wrote else " (h5py not importable: no .mcool)"))


if __name__ == "__main__":
    main()
