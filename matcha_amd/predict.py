"""Inference consumers of a trained classifier on the HIP forward.

* ``predict_multiway`` -- the flow of the reference's ``predict_multiway.py``: parse a text file of multi-way
  interactions (one per line, tab-separated ``chrom:position`` items), map positions to node ids through
  ``temp_dir/bin2node.npy``, score every hyperedge with ``model(x)`` in chunks of 10 000 rows zero-padded PER CHUNK
  (predict_multiway.py:74-87 -- a row's logit depends on the chunk's width because pads are attended, SURVEY.md headline
  fact 7, so the chunking is part of the result), sigmoid, ``np.savetxt``.
* ``pairwise_probabilities`` / ``proba2matrix`` -- the pairwise sweep of ``denoise_contact.py``: all intra-chromosome
  pairs (i, j >= i + min_distance) scored at k = 2 (:67-74, :147-153) and scattered into a symmetric matrix (:32-62).
  Pairs are generated and scored on the device (rows of one width are independent, so the 10 000-row chunks of the
  reference do not matter here); the .mcool writer, the coverage normalisation and the plots stay out of scope.

CLI:  python -m matcha_amd.predict multiway -i interactions.txt -o output.txt
      python -m matcha_amd.predict pairwise --chrom 0 -o chr1_proba.npy
      python -m matcha_amd.predict kway --chrom 0 --k 3 --top 1000 [--start-bin A --end-bin B] [--exclude-known] -o top.tsv
      python -m matcha_amd.predict anchored --k 3 --top 20 --chrom 5 (--anchor-file loci.tsv | --anchor-chrom 0) -o anchored.tsv
      python -m matcha_amd.predict complete -i clusters.txt --chrom 5 [--free 1] --top 20 [--width W] [--exclude-known] -o complete.tsv
      python -m matcha_amd.predict decompose -i clusters.txt --size 3 [--drop] [--min-gap G] --top 20 [--width W] [--exclude-known] [--pair-support] -o decompose.tsv
      python -m matcha_amd.predict grow -i seeds.txt --chrom 5 [--start-bin A --end-bin B] --max-size 10 [--beam 8] [--min-gap G] [--width W] [--exclude-known] -o grow.tsv
      python -m matcha_amd.predict regions --part 0:1 --part 5:1 --part 10:1:20-60 --top 1000 [--per-leading] [--map R C] [--exclude-known] -o regions.tsv
      python -m matcha_amd.predict kmap --chrom 0 --k 3 [--start-bin A --end-bin B] [--threshold 0.5] [--exclude-known] -o map.npz
      python -m matcha_amd.predict attention -i interactions.txt -o attn.npz [--per-head]
      python -m matcha_amd.predict outliers -i interactions.txt -o outliers.tsv [--lowest 3] [--scores scores.npz]
(all read ./config.JSON like the reference: temp_dir, resolution, chrom_list, min_distance).

* ``kway`` -- the de novo sweep of matcha_amd/sweep.py: every candidate of size k in one chromosome (or a window of its bins)
  with adjacent gaps > min_distance, scored on the device, the best ``--top`` written as ``chrom:start`` items and a probability.
* ``anchored`` -- the anchored sweep of matcha_amd/sweep.py: for every anchor (a line of ``--anchor-file``, or every bin of
  ``--anchor-chrom``) the best ``--top`` candidates of size k that contain it, the other nodes taken from ``--chrom``.
* ``complete`` -- cluster completion (matcha_amd/sweep.py): for every line of ``-i``, a cluster of 1 to 31 loci, the
  best ``--top`` bins (or sets of ``--free`` bins) of ``--chrom`` to add to it; per kept candidate the cluster's line number, the
  added loci and the probability.
* ``decompose`` -- cluster decomposition (matcha_amd/sweep.py): for every line of ``-i``, a cluster of 2 to 32 loci,
  the best ``--top`` sub-hyperedges of ``--size`` of its own loci, or with ``--drop`` the cluster with ``--size`` loci taken out; per
  kept candidate the cluster's line number, the chosen (kept or dropped) loci and the probability, with ``--drop`` also its change
  against the whole cluster.  ``<output>_support.tsv`` holds one line per cluster locus -- the mean probability and the number of the
  candidates whose choice contains it -- and a ``.npz`` beside them every returned tensor.  ``--pair-support`` (``--size`` >= 2) also
  writes ``<output>_pairs.npz``: per cluster the s x s block of the mean probability and the number of the candidates whose choice
  contains BOTH loci, in ``attention``'s ragged layout (``sizes``, ``offsets``, ``pair_mean``, ``pair_count``).
* ``grow`` -- cluster growth (matcha_amd/sweep.py): for every line of ``-i``, a seed of 1 to 31 loci, a beam search of
  the most plausible hubs of up to ``--max-size`` loci that contain it, one bin of ``--chrom`` added per step and ``--beam`` hubs kept
  per seed and size; per kept hub the seed's line number, the size, the loci and the probability, grouped by seed and size, best
  first, and a ``.npz`` beside it with every returned tensor.
* ``regions`` -- the multi-region sweep (matcha_amd/sweep.py): candidates with ``COUNT`` bins drawn from each ``--part
  CHROM:COUNT[:START-END]`` (a chromosome, or a window of its bins; parts in ascending genome order), e.g. every triple with one bin on
  each of three chromosomes; the best ``--top`` written like ``kway``'s, with ``--per-leading`` the best ``--top`` per candidate of the
  first part, grouped like ``anchored``'s; ``--map R C`` writes the pair map between parts R and C (R = C: within one part) to the
  ``.npz`` instead of a list.
* ``kmap`` -- the pair map of matcha_amd/sweep.py: the probabilities of ALL candidates of size k of one chromosome (or bin window)
  projected onto pairs of bins -- per pair the summed probability, the mean, the best candidate, the number of candidates and the
  number at or above ``--threshold`` -- written as one .npz of [n, n] matrices.
* ``attention`` -- ``attention_maps``: the lines of ``multiway``'s input (2 to 32 loci each), scored in the same chunks, and per line the
  k x k block of attention probabilities among its loci (``Classifier.get_embedding``), mean over the heads, as one .npz.
* ``outliers`` -- ``locus_scores``: the lines of ``multiway``'s input, scored in the same chunks; per line the
  probability, the size and the ``--lowest`` least supported loci as ``chrom:start`` with their scores (``Classifier.locus_scores``),
  ``--scores`` every locus's score as one .npz, ragged by line.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import utils as U

CHUNK_ROWS = 10000            # predict_multiway.py:77, denoise_contact.py:79


def parse_file(filepath: str, bin2node: Dict[str, int], chrom_list: Sequence[str], res: int, max_size: Optional[int] = None) -> List[List[int]]:
    """predict_multiway.py:24-59: items of unknown chromosomes are skipped, positions are floored to their bin, node ids
    are de-duplicated and sorted, lines with fewer than two nodes are dropped.  An item without ``:`` raises EOFError and
    an unknown bin raises KeyError, as in the reference.  ``max_size`` (not in the reference): a line with more distinct bins
    raises ValueError naming the 1-based line and its size."""
    final = []
    with open(filepath, "r") as f:
        for lineno, line in enumerate(f, 1):
            temp = []
            for info in line.strip().split("\t"):
                try:
                    chrom, bin_ = info.split(":")
                except ValueError:
                    raise EOFError(info)
                if chrom not in chrom_list:
                    continue
                b = int(math.floor(int(bin_) / res)) * res
                temp.append(bin2node["%s:%d" % (chrom, b)])
            temp = sorted(set(temp))
            if max_size is not None and len(temp) > max_size:
                raise ValueError("%s: line %d has %d distinct bins: model(x) scores rows of at most %d" % (filepath, lineno, len(temp), max_size))
            if len(temp) > 1:
                final.append(temp)
    return final


def predict(model, samples, batch_size: int = CHUNK_ROWS) -> np.ndarray:
    """Logits [n, 1] (numpy) of a list / array of hyperedges: eval mode, no grad, chunks of ``batch_size`` rows, each chunk
    zero-padded to ITS longest row (predict_multiway.py:74-87 == denoise_contact.py:76-88).  Rows of up to 32 nodes: a chunk wider
    than 8 takes the model's inference-only long forward; a longer row raises ValueError naming it, before anything is scored."""
    U.check_row_sizes(samples, _lib.MAX_LONG_L)
    model.eval()
    dev = model.layer_norm1.weight.device
    out = []
    with torch.no_grad():
        for j in range(0, len(samples), batch_size):
            x = U.pad_rows(samples[j:j + batch_size]).to(dev)
            out.append(model(x).detach().cpu().numpy())
    if not out:
        return np.zeros((0, 1), dtype=np.float32)
    return np.concatenate(out, axis=0)


def predict_multiway(model, filepath: str, bin2node: Dict[str, int], chrom_list: Sequence[str], res: int,
                     output: Optional[str] = None) -> Tuple[List[List[int]], np.ndarray]:
    """predict_multiway.py:104-113: parse, score, sigmoid, optionally ``np.savetxt`` (one probability per line).  Lines of up to 32
    distinct bins; a longer one fails with its line number before anything is scored."""
    samples = parse_file(filepath, bin2node, chrom_list, res, max_size=_lib.MAX_LONG_L)
    proba = torch.sigmoid(torch.from_numpy(predict(model, samples))).numpy()
    if output is not None:
        np.savetxt(output, proba)
    return samples, proba


def block_offsets(sizes: np.ndarray) -> np.ndarray:
    """int64 [n + 1]: where row i's k_i x k_i block starts in the ragged ``attn_mean`` of ``attention_maps`` (offsets[n]: its length)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(sizes * sizes)])


def attention_maps(model, samples, batch_size: int = CHUNK_ROWS, per_head: bool = False) -> Dict[str, np.ndarray]:
    """Which nodes of a hyperedge attend to which: the attention probabilities of ``model.get_embedding`` on a list / array of hyperedges of
    2 .. 32 nodes, reduced to the rows' REAL slots.  Chunks of ``batch_size`` rows, each zero-padded to ITS longest row exactly as ``predict``
    does it: padding slots are attended keys, so a row's probabilities depend on its chunk's width, and a row's block sums to less than 1 per
    query by what its pads received.  Returns numpy arrays

      sizes     int64 [n]        k_i, the nodes of row i
      offsets   int64 [n + 1]    block i is attn_mean[offsets[i]:offsets[i + 1]].reshape(k_i, k_i)
      attn_mean float32          the ragged blocks, row-major (query, key), mean over the eight heads
      attn_heads float32         per_head only: block i is attn_heads[8 * offsets[i]:8 * offsets[i + 1]].reshape(8, k_i, k_i)

    The head mean and the selection of the real slots run on the device, chunk by chunk; only the blocks come back.  A row of more than 32
    nodes raises ValueError naming it, before anything is scored."""
    U.check_row_sizes(samples, _lib.MAX_LONG_L)
    sizes, mean, heads = [], [], []
    if len(samples):
        model.eval()
        dev = model.layer_norm1.weight.device
        with torch.no_grad():
            for j in range(0, len(samples), batch_size):
                x = U.pad_rows(samples[j:j + batch_size]).to(dev)
                B, L = x.shape
                attn = model.get_embedding(x)[2].view(_lib.N_HEAD, B, L, L)
                real = x != 0
                pair = real.unsqueeze(2) & real.unsqueeze(1)                      # [B, L, L]: real query x real key
                sizes.append(real.sum(1).cpu().numpy().astype(np.int64))
                mean.append(attn.mean(0)[pair].cpu().numpy())                     # (b, query, key) order: row-major blocks, row after row
                if per_head:
                    heads.append(attn.permute(1, 0, 2, 3)[pair.unsqueeze(1).expand(B, _lib.N_HEAD, L, L)].cpu().numpy())
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    out = {"sizes": cat(sizes, np.int64)}
    out["offsets"] = block_offsets(out["sizes"])
    out["attn_mean"] = cat(mean, np.float32)
    if per_head:
        out["attn_heads"] = cat(heads, np.float32)
    return out


def locus_scores(model, samples, batch_size: int = CHUNK_ROWS, lowest: int = 3) -> Dict[str, np.ndarray]:
    """Which locus of each hyperedge the model supports least: ``Classifier.locus_scores`` on a list / array of hyperedges of 2 .. 32 nodes
    in ``predict``'s chunks -- file order, ``batch_size`` rows, each chunk zero-padded to ITS longest row -- so ``logit`` is ``predict``'s
    column row for row (the same bits where the chunk is wider than 8 and ``model(x)`` runs the same chain; to fp32 rounding where
    ``model(x)`` takes its short-row kernels).  Returns numpy arrays, ragged by hyperedge like ``attention_maps``'s:

      logit   float32 [n]      sizes  int64 [n]  k_i      offsets  int64 [n + 1]  row i's scores are scores[offsets[i]:offsets[i + 1]]
      scores  float32          the k_i per-locus scores of row i, in the row's node order
      lowest  int64 [n, lowest]  positions (0 .. k_i - 1) of the row's least supported loci, ascending by score; -1 behind the k_i-th

    A row of more than 32 nodes raises ValueError naming it, before anything is scored."""
    U.check_row_sizes(samples, _lib.MAX_LONG_L)
    lowest = int(lowest)
    logit, sizes, scores, low = [], [], [], []
    if len(samples):
        model.eval()
        dev = model.layer_norm1.weight.device
        with torch.no_grad():
            for j in range(0, len(samples), batch_size):
                x = U.pad_rows(samples[j:j + batch_size]).to(dev)
                if x.shape[1] < 2:
                    x = torch.nn.functional.pad(x, (0, 2 - x.shape[1]))
                res = model.locus_scores(x, lowest=lowest)
                real = x != 0
                logit.append(res.logits.view(-1).cpu().numpy())
                sizes.append(real.sum(1).cpu().numpy().astype(np.int64))
                scores.append(res.scores[real].cpu().numpy())
                if lowest:
                    # slot -> position among the row's real loci (the same thing for the zero-padded rows of pad_rows; kept general)
                    rank = torch.cumsum(real.long(), 1) - 1
                    o = res.order
                    low.append(torch.where(o >= 0, rank.gather(1, o.clamp(min=0)), o).cpu().numpy())
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    out = {"logit": cat(logit, np.float32), "sizes": cat(sizes, np.int64), "scores": cat(scores, np.float32)}
    out["offsets"] = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(out["sizes"])])
    out["lowest"] = np.concatenate(low) if low else np.zeros((0, lowest), dtype=np.int64)
    return out


def _outliers(args, config, temp_dir, model):
    bin2node = np.load(os.path.join(temp_dir, "bin2node.npy"), allow_pickle=True).item()
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    samples = parse_file(args.file, bin2node, config["chrom_list"], config["resolution"], max_size=_lib.MAX_LONG_L)
    out = locus_scores(model, samples, lowest=args.lowest)
    proba = torch.sigmoid(torch.from_numpy(out["logit"])).numpy()
    with open(args.output, "w") as f:
        for i, row in enumerate(samples):
            sc = out["scores"][out["offsets"][i]:out["offsets"][i + 1]]
            items = ["%s\t%r" % (node2bin[int(row[p])], float(sc[p])) for p in out["lowest"][i] if p >= 0]
            f.write("\t".join(["%.18e" % proba[i], str(len(row))] + items) + "\n")
    if args.scores:
        np.savez(args.scores, sizes=out["sizes"], offsets=out["offsets"], scores=out["scores"])
    print("%d interactions -> %s" % (len(samples), args.output))


def generate_pair_wise(chrom_range, chrom_id: int, min_dis: int, device=None) -> torch.Tensor:
    """All pairs (i, j) with start <= i, i + min_dis <= j < end of one chromosome, in the reference's order
    (denoise_contact.py:67-74), as an int64 [n, 2] tensor built on ``device`` (no host loop)."""
    lo, hi = int(chrom_range[chrom_id][0]), int(chrom_range[chrom_id][1])
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    cnt = torch.clamp(hi - i - int(min_dis), min=0)
    first = torch.repeat_interleave(i, cnt)
    start = torch.cumsum(cnt, 0) - cnt                                   # offset of each i's run
    j = torch.arange(int(cnt.sum()), dtype=torch.int64, device=device) - torch.repeat_interleave(start, cnt) + first + int(min_dis)
    return torch.stack([first, j], dim=1)


def pairwise_probabilities(model, chrom_range, chrom_id: int, min_dis: int, batch_rows: int = 1 << 20,
                           task_mode: str = "class") -> Tuple[torch.Tensor, torch.Tensor]:
    """(pairs int64 [n, 2], probabilities float32 [n]) on the model's device: sigmoid(model(pairs)) at width L = 2
    (denoise_contact.py:147-153); softplus(model(pairs)) for a model trained with task_mode 'regress' (:154-157)."""
    if task_mode not in ("class", "regress"):
        raise ValueError("task_mode must be 'class' or 'regress'")
    act = torch.nn.functional.softplus if task_mode == "regress" else torch.sigmoid
    model.eval()
    dev = model.layer_norm1.weight.device
    pairs = generate_pair_wise(chrom_range, chrom_id, min_dis, dev)
    out = torch.empty(len(pairs), dtype=torch.float32, device=dev)
    # back-to-back forwards: the per-call read-back of the device status word (one synchronisation each) is switched off and the
    # word is checked ONCE after the sweep (ids outside the model's tables are flagged on the device either way)
    check_each = getattr(model, "check_ids", None)
    if check_each is not None:
        model.check_ids = False
    try:
        with torch.no_grad():
            for s in range(0, len(pairs), batch_rows):
                out[s:s + batch_rows] = act(model(pairs[s:s + batch_rows].contiguous()).reshape(-1))
        if check_each is not None:
            model.check_status()            # IndexError if chrom_range does not belong to this model (ids beyond its tables)
    finally:
        if check_each is not None:
            model.check_ids = check_each
    return pairs, out


def proba2matrix(sample, weight=None, proba=None, intra: bool = True):
    """denoise_contact.py:32-62 for numpy arrays or torch tensors (the matrix is built where ``sample`` lives).
    intra: symmetric [size, size] with m[i, j] (+)= p for every pair of columns of ``sample`` (indices relative to the
    smallest id), then m + m.T; inter: [size1, size2] of the two columns.  ``weight``: p -> max(p * weight, p).
    Like the reference, repeated (i, j) do not accumulate (fancy-index ``+=``) and the caller's ``sample`` is untouched
    (the reference shifts its argument in place)."""
    is_np = isinstance(sample, np.ndarray)
    s = torch.as_tensor(sample).long()
    p = torch.as_tensor(proba, device=s.device).float()
    if weight is not None:
        p = torch.maximum(p * torch.as_tensor(weight, device=s.device).float(), p)
    if intra:
        s = s - s.min()
        size = int(s.max()) + 1
        m = torch.zeros(size, size, dtype=torch.float32, device=s.device)
        for i in range(s.shape[-1] - 1):
            for j in range(i + 1, s.shape[-1]):
                m[s[:, i], s[:, j]] = m[s[:, i], s[:, j]] + p
        m = m + m.T
    else:
        a, b = s[:, 0] - s[:, 0].min(), s[:, 1] - s[:, 1].min()
        m = torch.zeros(int(a.max()) + 1, int(b.max()) + 1, dtype=torch.float32, device=s.device)
        m[a, b] = m[a, b] + p
    return m.cpu().numpy() if is_np else m


def _load(config_path: str = "./config.JSON"):
    import json
    with open(config_path) as f:
        config = json.load(f)
    temp_dir = config["temp_dir"]
    model = torch.load(os.path.join(temp_dir, "model2load"), map_location="cuda", weights_only=False)   # main.py:322, :685
    return config, temp_dir, model


def _kway(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    c_lo, c_hi = int(chrom_range[args.chrom][0]), int(chrom_range[args.chrom][1])
    lo = c_lo + (args.start_bin if args.start_bin is not None else 0)
    hi = c_lo + args.end_bin if args.end_bin is not None else c_hi
    if not c_lo <= lo <= hi <= c_hi:
        raise ValueError("the bin window [%s, %s) is not inside chromosome %d (%d bins)" % (args.start_bin, args.end_bin, args.chrom, c_hi - c_lo))
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:
        known = np.load(os.path.join(temp_dir, "all_%d_counter.npy" % args.k)).astype(np.int64).reshape(-1, args.k)
        exclude = HyperedgeSet(torch.from_numpy(known).to(dev))
    min_gap = int(config["min_distance"]) + 1
    if args.enrich is not None:
        return _kway_enriched(args, model, chrom_range, node2bin, lo, hi, min_gap, exclude)
    out = SW.kway_sweep(model, lo, hi, args.k, min_gap, args.top, chunk_rows=args.chunk_rows, width=args.width,
                        exclude=exclude, task_mode=args.task_mode)
    rows, proba = out["rows"].cpu().numpy(), out["proba"].cpu().numpy()
    with open(args.output, "w") as f:
        for r, p in zip(rows, proba):
            f.write("\t".join([node2bin[int(v)] for v in r[:args.k]] + [repr(float(p))]) + "\n")
    np.savez(os.path.splitext(args.output)[0] + ".npz", rows=rows, logit=out["logit"].cpu().numpy(), proba=proba, rank=out["rank"].cpu().numpy())
    print("%d candidates (%d known, skipped) -> %d in %s" % (out["n_candidates"], out["n_excluded"], len(rows), args.output))


def parse_gap_edges(text: Optional[str]) -> Optional[Tuple[int, ...]]:
    """--gap-edges: a comma-separated, strictly ascending list of positive gaps ('' = no edges, one stratum); None = the default."""
    if text is None:
        return None
    try:
        edges = tuple(int(t) for t in text.split(",") if t.strip() != "")
    except ValueError:
        raise ValueError("--gap-edges must be a comma-separated list of integers (got %r)" % text)
    if any(e < 1 for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError("--gap-edges must be positive and strictly ascending (got %r)" % text)
    return edges


def _cli_expected(args, model, chrom_range, lo, hi, min_gap):
    """The expectation a --enrich run applies: --load-expected's file, or the expectation of every chromosome (--expected-chroms all), or
    None -- the sweep's own region, which kway_enriched_sweep computes itself (and whose logits it then keeps)."""
    from . import expected as EX
    if args.load_expected is not None:
        ex = EX.GapExpected.load(args.load_expected)
        if ex.k != args.k or ex.task_mode != args.task_mode:
            raise ValueError("%s holds the expectation of k=%d, task mode %s" % (args.load_expected, ex.k, ex.task_mode))
        return ex
    if args.expected_chroms == "all":
        regions = [(int(a), int(b)) for a, b in np.asarray(chrom_range)[:, :2]]
        return EX.kway_expected(model, regions, args.k, min_gap, edges=parse_gap_edges(args.gap_edges), width=args.width, chunk_rows=args.chunk_rows,
                                task_mode=args.task_mode, vmax=args.value_max)
    return None


def gap_ranges(decoded) -> str:
    """A stratum's gap ranges for the TSV: '1', '2-3', '8+' per gap, comma-separated."""
    return ",".join("%d+" % a if b is None else ("%d" % a if a == b else "%d-%d" % (a, b)) for a, b in decoded)


def _kway_enriched(args, model, chrom_range, node2bin, lo, hi, min_gap, exclude):
    from . import expected as EX
    ex = _cli_expected(args, model, chrom_range, lo, hi, min_gap)
    out = EX.kway_enriched_sweep(model, lo, hi, args.k, min_gap, args.top, expected=ex, mode=args.enrich, min_count=args.min_count,
                                 edges=parse_gap_edges(args.gap_edges), width=args.width, exclude=exclude, chunk_rows=args.chunk_rows,
                                 task_mode=args.task_mode, vmax=args.value_max)
    ex = out["expected_table"]
    if args.save_expected is not None:
        ex.save(args.save_expected)
    rows, proba, enrich = out["rows"].cpu().numpy(), out["proba"].cpu().numpy(), out["enrich"].cpu().numpy()
    stratum, mean = out["stratum"].cpu().numpy(), out["expected"].cpu().numpy()
    with open(args.output, "w") as f:
        for r, p, e, s, m in zip(rows, proba, enrich, stratum, mean):
            f.write("\t".join([node2bin[int(v)] for v in r[:args.k]] + [repr(float(p)), repr(float(e)), repr(float(m)), gap_ranges(ex.strata.decode(int(s)))])
                    + "\n")
    np.savez(os.path.splitext(args.output)[0] + ".npz", rows=rows, logit=out["logit"].cpu().numpy(), proba=proba, rank=out["rank"].cpu().numpy(),
             enrich=enrich, stratum=stratum, expected=mean, gap_edges=np.asarray(ex.edges, dtype=np.int64))
    print("%d candidates (%d known, skipped; %d in undersampled strata) -> %d by %s enrichment in %s"
          % (out["n_candidates"], out["n_excluded"], out["n_undersampled"], len(rows), args.enrich, args.output))


def _kmap(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    c_lo, c_hi = int(chrom_range[args.chrom][0]), int(chrom_range[args.chrom][1])
    lo = c_lo + (args.start_bin if args.start_bin is not None else 0)
    hi = c_lo + args.end_bin if args.end_bin is not None else c_hi
    if not c_lo <= lo <= hi <= c_hi:
        raise ValueError("the bin window [%s, %s) is not inside chromosome %d (%d bins)" % (args.start_bin, args.end_bin, args.chrom, c_hi - c_lo))
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:
        known = np.load(os.path.join(temp_dir, "all_%d_counter.npy" % args.k)).astype(np.int64).reshape(-1, args.k)
        exclude = HyperedgeSet(torch.from_numpy(known).to(dev))
    min_gap = int(config["min_distance"]) + 1
    extra = {}
    if args.enrich is not None:                                          # the observed-over-expected map
        from . import expected as EX
        ex = _cli_expected(args, model, chrom_range, lo, hi, min_gap)
        if ex is None:
            ex = EX.kway_expected(model, [(lo, hi)], args.k, min_gap, edges=parse_gap_edges(args.gap_edges), width=args.width,
                                  chunk_rows=args.chunk_rows, task_mode=args.task_mode, vmax=args.value_max)
        if args.save_expected is not None:
            ex.save(args.save_expected)
        extra = dict(expected=ex, mode=args.enrich, min_count=args.min_count)
    out = SW.kway_map(model, lo, hi, args.k, min_gap, chunk_rows=args.chunk_rows, width=args.width, exclude=exclude, task_mode=args.task_mode,
                      threshold=args.threshold, value_max=None if args.enrich is not None else args.value_max, **extra)      # a ratio's cap is kway_map's default, 1024
    if args.enrich is not None:
        extra = dict(gap_edges=np.asarray(ex.edges, dtype=np.int64), expected_mean=ex.mean, expected_count=ex.count, min_count=np.int64(args.min_count))
    np.savez(args.output, **{name: out[name].cpu().numpy() for name in ("sum", "mean", "max", "count", "count_ge")}, lo=np.int64(lo),
             n=np.int64(hi - lo), k=np.int64(args.k), min_gap=np.int64(min_gap), threshold=np.float32(args.threshold), **extra)
    print("%d candidates (%d known, skipped; %d rejected) -> %d x %d map in %s"
          % (out["n_candidates"], out["n_excluded"], out["n_rejected"], hi - lo, hi - lo, args.output))


def parse_parts(specs: Sequence[str], chrom_range, chrom_list: Sequence[str]) -> List[Tuple[int, int, int]]:
    """[(lo, hi, m)] in node ids from ``--part CHROM:COUNT[:START-END]`` arguments: CHROM an index into chrom_list or one of its names,
    COUNT >= 1 bins drawn from the part, START-END a window of bins relative to the chromosome (default: all of it).  The parts must
    come in ascending genome order without overlap; every error is a ValueError that names the offending argument."""
    if not specs:
        raise ValueError("regions needs at least one --part CHROM:COUNT[:START-END]")
    names = list(chrom_list)
    parts = []
    for spec in specs:
        what = "--part %s" % spec
        items = spec.split(":")
        if len(items) not in (2, 3):
            raise ValueError("%s: expected CHROM:COUNT or CHROM:COUNT:START-END" % what)
        if items[0] in names:
            chrom = names.index(items[0])
        else:
            try:
                chrom = int(items[0])
            except ValueError:
                raise ValueError("%s: %r is neither a name nor an index of chrom_list" % (what, items[0]))
        if not 0 <= chrom < len(chrom_range):
            raise ValueError("%s: chromosome index %d outside [0, %d)" % (what, chrom, len(chrom_range)))
        try:
            m = int(items[1])
        except ValueError:
            raise ValueError("%s: COUNT %r is not an integer" % (what, items[1]))
        if m < 1:
            raise ValueError("%s: COUNT must be >= 1" % what)
        c_lo, c_hi = int(chrom_range[chrom][0]), int(chrom_range[chrom][1])
        lo, hi = c_lo, c_hi
        if len(items) == 3:
            try:
                start, end = (int(v) for v in items[2].split("-"))
            except ValueError:
                raise ValueError("%s: the window %r is not START-END" % (what, items[2]))
            lo, hi = c_lo + start, c_lo + end
            if not c_lo <= lo < hi <= c_hi:
                raise ValueError("%s: the bin window [%d, %d) is empty or not inside the chromosome (%d bins)" % (what, start, end, c_hi - c_lo))
        if parts and lo < parts[-1][1]:
            raise ValueError("%s: parts must be given in ascending genome order without overlap (it begins at node %d, the part before "
                             "ends at %d)" % (what, lo, parts[-1][1]))
        parts.append((lo, hi, m))
    return parts


def _regions(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    parts = parse_parts(args.part, chrom_range, config["chrom_list"])
    k = sum(m for _, _, m in parts)
    min_gap = args.min_gap if args.min_gap is not None else int(config["min_distance"]) + 1
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:
        known = np.load(os.path.join(temp_dir, "all_%d_counter.npy" % k)).astype(np.int64).reshape(-1, k)
        exclude = HyperedgeSet(torch.from_numpy(known).to(dev))
    npz = os.path.splitext(args.output)[0] + ".npz"
    if args.map is not None:
        r, c = args.map
        out = SW.region_map(model, parts, min_gap, r, c, chunk_rows=args.chunk_rows, width=args.width, exclude=exclude, task_mode=args.task_mode,
                            threshold=args.threshold, value_max=args.value_max)
        np.savez(npz, **{name: out[name].cpu().numpy() for name in ("sum", "mean", "max", "count", "count_ge")},
                 parts=np.asarray(parts, dtype=np.int64), rows_part=np.int64(r), cols_part=np.int64(c), min_gap=np.int64(min_gap),
                 threshold=np.float32(args.threshold))
        print("%d candidates (%d against the gap rule, %d known, skipped; %d rejected) -> %d x %d map in %s"
              % (out["n_candidates"], out["n_invalid"], out["n_excluded"], out["n_rejected"], parts[r][1] - parts[r][0], parts[c][1] - parts[c][0], npz))
        return
    if args.top is None:
        raise ValueError("regions needs --top (or --map R C)")
    out = SW.region_sweep(model, parts, min_gap, args.top, chunk_rows=args.chunk_rows, width=args.width, exclude=exclude,
                          task_mode=args.task_mode, per_leading=args.per_leading)
    rows, proba = out["rows"].cpu().numpy(), out["proba"].cpu().numpy()
    extra = {}
    with open(args.output, "w") as f:
        if args.per_leading:
            count = out["count"].cpu().numpy()
            extra = dict(count=count, leading=out["leading"].cpu().numpy())
            kept = int(count.sum())
            for a in range(len(count)):                                  # grouped by the leading candidate, best first
                for r, p in zip(rows[a, :count[a]], proba[a, :count[a]]):
                    f.write("\t".join([node2bin[int(v)] for v in r[:k]] + [repr(float(p))]) + "\n")
        else:
            kept = len(rows)
            for r, p in zip(rows, proba):
                f.write("\t".join([node2bin[int(v)] for v in r[:k]] + [repr(float(p))]) + "\n")
    np.savez(npz, rows=rows, logit=out["logit"].cpu().numpy(), proba=proba, rank=out["rank"].cpu().numpy(), **extra)
    print("%d candidates (%d against the gap rule, %d known, skipped) -> %d in %s"
          % (out["n_candidates"], out["n_invalid"], out["n_excluded"], kept, args.output))


def parse_anchor_file(filepath: str, bin2node: Dict[str, int], chrom_list: Sequence[str], res: int) -> np.ndarray:
    """int64 [A, s]: one anchor row per non-empty line, s tab-separated ``chrom:position`` loci with parse_file's coordinate
    handling (positions floored to their bin, an item without ``:`` raises EOFError, an unknown bin KeyError), each row sorted.
    Unlike parse_file nothing is dropped: a locus of an unknown chromosome, a repeated locus or lines of different lengths raise
    ValueError, because every line is one anchor and all anchors share s."""
    rows = []
    with open(filepath, "r") as f:
        for line in f:
            if not line.strip():
                continue
            temp = []
            for info in line.strip().split("\t"):
                try:
                    chrom, bin_ = info.split(":")
                except ValueError:
                    raise EOFError(info)
                if chrom not in chrom_list:
                    raise ValueError("anchor locus %s: chromosome not in chrom_list" % info)
                b = int(math.floor(int(bin_) / res)) * res
                temp.append(bin2node["%s:%d" % (chrom, b)])
            if len(set(temp)) != len(temp):
                raise ValueError("anchor line %r repeats a bin" % line.strip())
            rows.append(sorted(temp))
    if len(set(len(r) for r in rows)) > 1:
        raise ValueError("all anchor lines must have the same number of loci")
    return np.asarray(rows, dtype=np.int64).reshape(len(rows), len(rows[0]) if rows else 1)


def _anchored(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()

    def window(chrom, start_bin, end_bin):
        c_lo, c_hi = int(chrom_range[chrom][0]), int(chrom_range[chrom][1])
        lo = c_lo + (start_bin if start_bin is not None else 0)
        hi = c_lo + end_bin if end_bin is not None else c_hi
        if not c_lo <= lo <= hi <= c_hi:
            raise ValueError("the bin window [%s, %s) is not inside chromosome %d (%d bins)" % (start_bin, end_bin, chrom, c_hi - c_lo))
        return lo, hi

    lo, hi = window(args.chrom, args.start_bin, args.end_bin)
    if args.anchor_file is not None:
        bin2node = {v: key for key, v in node2bin.items()}
        anchors = parse_anchor_file(args.anchor_file, bin2node, config["chrom_list"], config["resolution"])
    else:
        a_lo, a_hi = window(args.anchor_chrom, args.anchor_start_bin, args.anchor_end_bin)
        anchors = np.arange(a_lo, a_hi, dtype=np.int64).reshape(-1, 1)
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:
        known = np.load(os.path.join(temp_dir, "all_%d_counter.npy" % args.k)).astype(np.int64).reshape(-1, args.k)
        exclude = HyperedgeSet(torch.from_numpy(known).to(dev))
    out = SW.anchored_sweep(model, anchors, lo, hi, args.k, int(config["min_distance"]) + 1, args.top, chunk_rows=args.chunk_rows,
                            width=args.width, exclude=exclude, task_mode=args.task_mode)
    rows, proba, count = out["rows"].cpu().numpy(), out["proba"].cpu().numpy(), out["count"].cpu().numpy()
    with open(args.output, "w") as f:
        for a in range(len(anchors)):
            for r, p in zip(rows[a, :count[a]], proba[a, :count[a]]):
                f.write("\t".join([node2bin[int(v)] for v in r[:args.k]] + [repr(float(p))]) + "\n")
    np.savez(os.path.splitext(args.output)[0] + ".npz", anchors=anchors, rows=rows, logit=out["logit"].cpu().numpy(), proba=proba,
             rank=out["rank"].cpu().numpy(), count=count)
    print("%d anchors, %d candidates (%d against the gap rule, %d known, skipped) -> %d in %s"
          % (len(anchors), out["n_candidates"], out["n_invalid"], out["n_excluded"], int(count.sum()), args.output))


def parse_cluster_file(filepath: str, bin2node: Dict[str, int], chrom_list: Sequence[str], res: int, free: int = 1,
                       least: int = 1, most: Optional[int] = None) -> Tuple[List[List[int]], List[int]]:
    """(clusters, line numbers): one cluster per line, 1 to 31 tab-separated ``chrom:position`` loci with parse_file's coordinate
    handling (items of unknown chromosomes are skipped, positions floored to their bin, node ids de-duplicated and sorted; an item
    without ``:`` raises EOFError, an unknown bin KeyError).  Lines may differ in length; a line that leaves no locus is dropped.  A
    line with more than 31 distinct bins, or with more than 32 - free, raises ValueError naming its 1-based number.  ``least`` /
    ``most`` (``decompose``: 2 and 32) replace those bounds: a line with a locus but fewer than ``least`` distinct bins raises too."""
    given = most is not None
    most = min(_lib.MAX_LONG_L - 1, _lib.MAX_LONG_L - int(free)) if most is None else int(most)
    clusters, lines = [], []
    with open(filepath, "r") as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            temp = []
            for info in line.strip().split("\t"):
                try:
                    chrom, bin_ = info.split(":")
                except ValueError:
                    raise EOFError(info)
                if chrom not in chrom_list:
                    continue
                b = int(math.floor(int(bin_) / res)) * res
                temp.append(bin2node["%s:%d" % (chrom, b)])
            temp = sorted(set(temp))
            if given and temp and not least <= len(temp) <= most:
                raise ValueError("%s: line %d has %d distinct bins: a cluster holds %d to %d" % (filepath, lineno, len(temp), least, most))
            if len(temp) > most:
                raise ValueError("%s: line %d has %d distinct bins: a cluster completed by %d free bin(s) holds at most %d"
                                 % (filepath, lineno, len(temp), int(free), most))
            if temp:
                clusters.append(temp)
                lines.append(lineno)
    return clusters, lines


def _complete(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    if not 1 <= args.free <= _lib.MAX_L:
        raise ValueError("--free must be in 1 .. %d" % _lib.MAX_L)
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    bin2node = {v: key for key, v in node2bin.items()}
    clusters, lines = parse_cluster_file(args.file, bin2node, config["chrom_list"], config["resolution"], args.free)      # before anything is scored
    c_lo, c_hi = int(chrom_range[args.chrom][0]), int(chrom_range[args.chrom][1])
    lo = c_lo + (args.start_bin if args.start_bin is not None else 0)
    hi = c_lo + args.end_bin if args.end_bin is not None else c_hi
    if not c_lo <= lo <= hi <= c_hi:
        raise ValueError("the bin window [%s, %s) is not inside chromosome %d (%d bins)" % (args.start_bin, args.end_bin, args.chrom, c_hi - c_lo))
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:      # a candidate of a cluster of s loci has s + free: every size present, one set (rows of all sizes share a table)
        known = []
        for k in sorted({len(c) + args.free for c in clusters}):
            path = os.path.join(temp_dir, "all_%d_counter.npy" % k)
            if os.path.exists(path):
                rows = np.load(path).astype(np.int64).reshape(-1, k)
                known.append(np.pad(rows, ((0, 0), (0, _lib.MAX_LONG_L - k))))
        if not known:
            raise FileNotFoundError("--exclude-known: no all_<k>_counter.npy in %s for the candidate sizes of %s" % (temp_dir, args.file))
        exclude = HyperedgeSet(torch.from_numpy(np.concatenate(known)).to(dev))
    table = np.zeros((len(clusters), max([len(c) for c in clusters] + [1])), dtype=np.int64)
    for a, c in enumerate(clusters):
        table[a, :len(c)] = c
    out = SW.completion_sweep(model, table, lo, hi, free=args.free, min_gap=int(config["min_distance"]) + 1, top=args.top,
                              chunk_rows=args.chunk_rows, width=args.width, exclude=exclude, task_mode=args.task_mode)
    rows, added, proba, count = out["rows"].cpu().numpy(), out["added"].cpu().numpy(), out["proba"].cpu().numpy(), out["count"].cpu().numpy()
    with open(args.output, "w") as f:
        for a in range(len(clusters)):
            for ids, p in zip(added[a, :count[a]], proba[a, :count[a]]):
                f.write("\t".join([str(lines[a])] + [node2bin[int(v)] for v in ids] + [repr(float(p))]) + "\n")
    np.savez(os.path.splitext(args.output)[0] + ".npz", clusters=table, rows=rows, added=added, logit=out["logit"].cpu().numpy(), proba=proba,
             rank=out["rank"].cpu().numpy(), count=count)
    print("%d anchors, %d candidates (%d against the gap rule, %d known, skipped) -> %d in %s"
          % (len(clusters), out["n_candidates"], out["n_invalid"], out["n_excluded"], int(count.sum()), args.output))


def _grow(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    if not 2 <= args.max_size <= _lib.MAX_LONG_L:
        raise ValueError("--max-size must be in 2 .. %d" % _lib.MAX_LONG_L)
    if not 1 <= args.beam <= SW.MAX_BEAM:
        raise ValueError("--beam must be in 1 .. %d" % SW.MAX_BEAM)
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    bin2node = {v: key for key, v in node2bin.items()}
    seeds, lines = parse_cluster_file(args.file, bin2node, config["chrom_list"], config["resolution"])      # before anything is scored
    c_lo, c_hi = int(chrom_range[args.chrom][0]), int(chrom_range[args.chrom][1])
    lo = c_lo + (args.start_bin if args.start_bin is not None else 0)
    hi = c_lo + args.end_bin if args.end_bin is not None else c_hi
    if not c_lo <= lo <= hi <= c_hi:
        raise ValueError("the bin window [%s, %s) is not inside chromosome %d (%d bins)" % (args.start_bin, args.end_bin, args.chrom, c_hi - c_lo))
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:      # a seed of s loci passes through every size s + 1 .. max_size: every size present, one set
        known = []
        for k in sorted({k for c in seeds for k in range(len(c) + 1, args.max_size + 1)}):
            path = os.path.join(temp_dir, "all_%d_counter.npy" % k)
            if os.path.exists(path):
                rows = np.load(path).astype(np.int64).reshape(-1, k)
                known.append(np.pad(rows, ((0, 0), (0, _lib.MAX_LONG_L - k))))
        if not known:
            raise FileNotFoundError("--exclude-known: no all_<k>_counter.npy in %s for the hub sizes of %s" % (temp_dir, args.file))
        exclude = HyperedgeSet(torch.from_numpy(np.concatenate(known)).to(dev))
    table = np.zeros((len(seeds), max([len(c) for c in seeds] + [1])), dtype=np.int64)
    for a, c in enumerate(seeds):
        table[a, :len(c)] = c
    min_gap = int(config["min_distance"]) + 1 if args.min_gap is None else args.min_gap
    out = SW.growth_sweep(model, table, lo, hi, args.max_size, beam=args.beam, min_gap=min_gap, width=args.width, exclude=exclude,
                          chunk_rows=args.chunk_rows, task_mode=args.task_mode)
    z = {key: out[key].cpu().numpy() for key in ("rows", "logit", "proba", "parent", "added", "count", "size", "path")}
    with open(args.output, "w") as f:
        for a in range(len(seeds)):
            for t in range(z["count"].shape[1]):
                for ids, p in zip(z["rows"][a, t, :z["count"][a, t]], z["proba"][a, t, :z["count"][a, t]]):
                    f.write("\t".join([str(lines[a]), str(int(z["size"][a, t]))] + [node2bin[int(v)] for v in ids if v] + [repr(float(p))]) + "\n")
    np.savez(os.path.splitext(args.output)[0] + ".npz", seeds=table, **z)
    print("%d seeds, %d steps, %d candidates (%d against the gap rule, %d twins, %d known, skipped) -> %d in %s"
          % (len(seeds), out["steps"], out["n_candidates"], out["n_invalid"], out["n_twins"], out["n_excluded"], int(z["count"].sum()), args.output))


def _decompose(args, config, temp_dir, model):
    from . import sweep as SW
    from .sampler import HyperedgeSet
    if not (1 if args.drop else 2) <= args.size <= _lib.MAX_L:
        raise ValueError("--size must be in %d .. %d" % (1 if args.drop else 2, _lib.MAX_L))
    if args.pair_support and args.size < 2:
        raise ValueError("--pair-support needs --size >= 2: a choice of one locus has no pair")
    node2bin = np.load(os.path.join(temp_dir, "node2bin.npy"), allow_pickle=True).item()
    bin2node = {v: key for key, v in node2bin.items()}
    clusters, lines = parse_cluster_file(args.file, bin2node, config["chrom_list"], config["resolution"], least=2,
                                         most=_lib.MAX_LONG_L)                                  # before anything is scored
    dev = model.layer_norm1.weight.device
    exclude = None
    if args.exclude_known:      # a candidate of a cluster of s loci has --size loci (keep) or s - size (drop): every size present, one set
        known = []
        for k in sorted({len(c) - args.size for c in clusters} if args.drop else {args.size}):
            path = os.path.join(temp_dir, "all_%d_counter.npy" % k)
            if k >= 2 and os.path.exists(path):
                rows = np.load(path).astype(np.int64).reshape(-1, k)
                known.append(np.pad(rows, ((0, 0), (0, _lib.MAX_LONG_L - k))))
        if not known:
            raise FileNotFoundError("--exclude-known: no all_<k>_counter.npy in %s for the candidate sizes of %s" % (temp_dir, args.file))
        exclude = HyperedgeSet(torch.from_numpy(np.concatenate(known)).to(dev))
    table = np.zeros((len(clusters), max([len(c) for c in clusters] + [2])), dtype=np.int64)
    for a, c in enumerate(clusters):
        table[a, :len(c)] = c
    min_gap = int(config["min_distance"]) + 1 if args.min_gap is None else args.min_gap
    out = SW.decomposition_sweep(model, table, args.size, mode="drop" if args.drop else "keep", min_gap=min_gap, top=args.top,
                                 chunk_rows=args.chunk_rows, width=args.width, exclude=exclude, pair_support=args.pair_support)
    z = {key: v.cpu().numpy() for key, v in out.items() if isinstance(v, torch.Tensor) and not key.startswith("pair_")}
    count = z["count"]
    with open(args.output, "w") as f:
        for a in range(len(clusters)):
            for ids, p in zip(z["chosen"][a, :count[a]], z["proba"][a, :count[a]]):
                cells = [str(lines[a])] + [node2bin[int(v)] for v in ids] + [repr(float(p))]
                if args.drop:
                    cells.append(repr(float(p) - float(z["full_proba"][a])))
                f.write("\t".join(cells) + "\n")
    base = os.path.splitext(args.output)[0]
    with open(base + "_support.tsv", "w") as f:
        for a, c in enumerate(clusters):
            for j, v in enumerate(c):
                f.write("\t".join([str(lines[a]), node2bin[int(v)], repr(float(z["support_mean"][a, j])), str(int(z["support_count"][a, j]))]) + "\n")
    np.savez(base + ".npz", clusters=table, **z)
    if args.pair_support:       # attention_maps' layout: cluster a is the row-major s_a x s_a block at offsets[a], loci in the order of _support.tsv
        sizes = np.asarray([len(c) for c in clusters], dtype=np.int64)
        mean, cnt = out["pair_mean"].cpu().numpy(), out["pair_count"].cpu().numpy()
        flat = lambda t, dtype: np.concatenate([t[a, :s, :s].reshape(-1) for a, s in enumerate(sizes)] + [np.zeros(0, dtype=dtype)]).astype(dtype)
        np.savez(base + "_pairs.npz", sizes=sizes, offsets=block_offsets(sizes), pair_mean=flat(mean, np.float32), pair_count=flat(cnt, np.int64))
    print("%d clusters, %d candidates (%d against the gap rule, %d known, skipped) -> %d in %s"
          % (len(clusters), out["n_candidates"], out["n_invalid"], out["n_excluded"], int(count.sum()), args.output))


def main(argv=None):
    ap = argparse.ArgumentParser(description="inference consumers of a trained MATCHA classifier on the MI355X path")
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("multiway", help="predict_multiway.py: probabilities of the multi-way interactions of a text file")
    a.add_argument("-i", "--file", type=str, required=True)
    a.add_argument("-o", "--output", type=str, default="./output.txt")
    b = sub.add_parser("pairwise", help="denoise_contact.py's sweep: probability matrix of all intra-chromosome pairs")
    b.add_argument("--chrom", type=int, required=True, help="index into config chrom_list")
    b.add_argument("-o", "--output", type=str, default="./pairwise.npy")
    b.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    c = sub.add_parser("kway", help="de novo sweep: the best --top candidates of size --k among all of one chromosome (or bin window)")
    c.add_argument("--chrom", type=int, required=True, help="index into config chrom_list")
    c.add_argument("--k", type=int, required=True, help="candidate size, 2 .. 8")
    c.add_argument("--top", type=int, required=True, help="how many candidates to keep")
    c.add_argument("--start-bin", type=int, default=None, help="first bin of the window, relative to the chromosome (default 0)")
    c.add_argument("--end-bin", type=int, default=None, help="one past the last bin of the window (default: the chromosome's end)")
    c.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy")
    c.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default k): a logit depends on its batch's width")
    c.add_argument("--chunk-rows", type=int, default=1 << 20)
    c.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    c.add_argument("-o", "--output", type=str, default="./kway.tsv")
    c.add_argument("--enrich", choices=["logodds", "ratio", "z"], default=None,
                   help="rank by enrichment over the distance-matched expectation instead of by probability; adds the columns enrich, expected and gap ranges")
    c.add_argument("--value-max", type=float, default=None, help="--enrich with task-mode regress: the largest value the expectation accepts (<= 2^20)")
    d = sub.add_parser("anchored", help="anchored sweep: for every anchor the best --top candidates of size --k that contain it")
    d.add_argument("--chrom", type=int, required=True, help="the partner region: index into config chrom_list")
    d.add_argument("--k", type=int, required=True, help="candidate size, 2 .. 8 (anchor loci included)")
    d.add_argument("--top", type=int, required=True, help="how many candidates to keep per anchor")
    src = d.add_mutually_exclusive_group(required=True)
    src.add_argument("--anchor-file", type=str, default=None, help="one anchor per line: s tab-separated chrom:position loci, the same s on every line")
    src.add_argument("--anchor-chrom", type=int, default=None, help="every bin of this chromosome (or of its --anchor-*-bin window) as a single anchor")
    d.add_argument("--anchor-start-bin", type=int, default=None, help="first anchor bin, relative to --anchor-chrom (default 0)")
    d.add_argument("--anchor-end-bin", type=int, default=None, help="one past the last anchor bin (default: the chromosome's end)")
    d.add_argument("--start-bin", type=int, default=None, help="first bin of the partner window, relative to --chrom (default 0)")
    d.add_argument("--end-bin", type=int, default=None, help="one past the last bin of the partner window (default: the chromosome's end)")
    d.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy")
    d.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default k): a logit depends on its batch's width")
    d.add_argument("--chunk-rows", type=int, default=1 << 20)
    d.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    d.add_argument("-o", "--output", type=str, default="./anchored.tsv")
    h = sub.add_parser("complete", help="cluster completion: for every cluster of 1 .. 31 loci the best --top bins (or sets of --free bins) to add")
    h.add_argument("-i", "--file", type=str, required=True, help="one cluster per line: 1 .. 31 tab-separated chrom:position loci; lines may differ in length")
    h.add_argument("--chrom", type=int, required=True, help="the partner region: index into config chrom_list")
    h.add_argument("--start-bin", type=int, default=None, help="first bin of the partner window, relative to --chrom (default 0)")
    h.add_argument("--end-bin", type=int, default=None, help="one past the last bin of the partner window (default: the chromosome's end)")
    h.add_argument("--free", type=int, default=1, help="how many bins to add to each cluster, 1 .. 8")
    h.add_argument("--top", type=int, required=True, help="how many candidates to keep per cluster")
    h.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default: longest cluster + free, at most 32)")
    h.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy, for every candidate size k present")
    h.add_argument("--chunk-rows", type=int, default=None, help="rows per forward (default: 2^20 up to width 8, min(2^20, 2^21 // width) beyond)")
    h.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    h.add_argument("-o", "--output", type=str, default="./complete.tsv")
    h.add_argument("--config", type=str, default="./config.JSON")
    m = sub.add_parser("grow", help="cluster growth: beam-search the most plausible hubs of up to --max-size loci that contain each seed of 1 .. 31 loci")
    m.add_argument("-i", "--file", type=str, required=True, help="one seed per line: 1 .. 31 tab-separated chrom:position loci; lines may differ in length")
    m.add_argument("--chrom", type=int, required=True, help="the region the added bins come from: index into config chrom_list")
    m.add_argument("--start-bin", type=int, default=None, help="first bin of the window, relative to --chrom (default 0)")
    m.add_argument("--end-bin", type=int, default=None, help="one past the last bin of the window (default: the chromosome's end)")
    m.add_argument("--max-size", type=int, required=True, help="grow every seed up to this many loci, 2 .. 32")
    m.add_argument("--beam", type=int, default=8, help="hubs kept per seed and size, 1 .. 64")
    m.add_argument("--min-gap", type=int, default=None, help="smallest difference of adjacent node ids in a hub (default: min_distance + 1)")
    m.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default: --max-size, at most 32): every step is scored at one width")
    m.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy, for every hub size k present")
    m.add_argument("--chunk-rows", type=int, default=None, help="rows per forward (default: 2^20 up to width 8, min(2^20, 2^21 // width) beyond)")
    m.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    m.add_argument("-o", "--output", type=str, default="./grow.tsv")
    m.add_argument("--config", type=str, default="./config.JSON")
    k = sub.add_parser("decompose", help="cluster decomposition: the best --top sub-hyperedges of --size loci of every cluster of 2 .. 32 loci, or (--drop) the cluster without them")
    k.add_argument("-i", "--file", type=str, required=True, help="one cluster per line: 2 .. 32 tab-separated chrom:position loci; lines may differ in length")
    k.add_argument("--size", type=int, required=True, help="how many of the cluster's loci a candidate keeps (2 .. 8) or, with --drop, leaves out (1 .. 8)")
    k.add_argument("--drop", action="store_true", help="score the cluster with --size loci taken out, beside the whole cluster")
    k.add_argument("--min-gap", type=int, default=None, help="smallest difference of adjacent node ids in a candidate (default: min_distance + 1)")
    k.add_argument("--top", type=int, required=True, help="how many candidates to keep per cluster")
    k.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default: --size, at most 8; --drop: the longest cluster, at most 32)")
    k.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy, for every candidate size k present")
    k.add_argument("--chunk-rows", type=int, default=None, help="rows per forward (default: 2^20 up to width 8, min(2^20, 2^21 // width) beyond)")
    k.add_argument("--pair-support", action="store_true", help="also write <output>_pairs.npz: per cluster the s x s mean probability and number of the candidates that contain both loci (--size >= 2)")
    k.add_argument("-o", "--output", type=str, default="./decompose.tsv")
    k.add_argument("--config", type=str, default="./config.JSON")
    r = sub.add_parser("regions", help="multi-region sweep: the best --top candidates with bins drawn from several chromosomes or bin windows")
    r.add_argument("--part", action="append", default=[], metavar="CHROM:COUNT[:START-END]",
                   help="repeatable, 1 .. 8 times in ascending genome order: COUNT bins drawn from chromosome CHROM (index into config chrom_list, "
                        "or its name), or from its bins START .. END - 1")
    r.add_argument("--top", type=int, default=None, help="how many candidates to keep (with --per-leading: per candidate of the first part)")
    r.add_argument("--min-gap", type=int, default=None, help="smallest difference of adjacent node ids in a candidate (default: min_distance + 1)")
    r.add_argument("--per-leading", action="store_true", help="keep the best --top for every candidate of the first part (needs two parts or more)")
    r.add_argument("--map", type=int, nargs=2, default=None, metavar=("R", "C"),
                   help="write the pair map between the bins of parts R and C (R = C: within one part) to the .npz instead of a list")
    r.add_argument("--threshold", type=float, default=0.5, help="--map: count_ge counts the candidates of a pair with a value >= this")
    r.add_argument("--value-max", type=float, default=None, help="--map with task-mode regress: the largest value a candidate may contribute (<= 2^20)")
    r.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy")
    r.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default k): a logit depends on its batch's width")
    r.add_argument("--chunk-rows", type=int, default=1 << 20)
    r.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    r.add_argument("-o", "--output", type=str, default="./regions.tsv")
    r.add_argument("--config", type=str, default="./config.JSON")
    e = sub.add_parser("kmap", help="pair map: the probabilities of all candidates of size --k projected onto pairs of bins")
    e.add_argument("--chrom", type=int, required=True, help="index into config chrom_list")
    e.add_argument("--k", type=int, required=True, help="candidate size, 2 .. 8")
    e.add_argument("--start-bin", type=int, default=None, help="first bin of the window, relative to the chromosome (default 0)")
    e.add_argument("--end-bin", type=int, default=None, help="one past the last bin of the window (default: the chromosome's end)")
    e.add_argument("--threshold", type=float, default=0.5, help="count_ge counts the candidates of a pair with a value >= this")
    e.add_argument("--exclude-known", action="store_true", help="skip the hyperedges of temp_dir/all_<k>_counter.npy")
    e.add_argument("--width", type=int, default=None, help="zero-pad rows to this width (default k): a logit depends on its batch's width")
    e.add_argument("--chunk-rows", type=int, default=1 << 20)
    e.add_argument("--task-mode", choices=["class", "regress"], default="class", help="the model's training objective: sigmoid or softplus outputs")
    e.add_argument("--value-max", type=float, default=None, help="task-mode regress: the largest value a candidate may contribute (<= 2^20); with --enrich: the largest the expectation accepts (a ratio's cap is 1024)")
    e.add_argument("-o", "--output", type=str, default="./kmap.npz")
    e.add_argument("--enrich", choices=["ratio"], default=None, help="the observed-over-expected map: every candidate's value divided by the mean of its gap stratum")
    for q in (c, e):
        q.add_argument("--gap-edges", type=str, default=None, help="--enrich: the gap classes' edges, comma-separated and ascending (default: powers of two)")
        q.add_argument("--min-count", type=int, default=30, help="--enrich: strata with fewer candidates have no expectation; their candidates drop out")
        q.add_argument("--expected-chroms", choices=["all", "same"], default="same",
                       help="--enrich: take the expectation over every chromosome (the Hi-C convention) or over the swept window only")
        q.add_argument("--save-expected", type=str, default=None, help="--enrich: write the expectation to this .npz")
        q.add_argument("--load-expected", type=str, default=None, help="--enrich: apply the expectation of this .npz instead of computing one")
    g = sub.add_parser("attention", help="attention maps: per interaction of a text file, the head-mean attention among its loci")
    g.add_argument("-i", "--file", type=str, required=True)
    g.add_argument("-o", "--output", type=str, default="./attn.npz")
    g.add_argument("--per-head", action="store_true", help="also write the eight heads' blocks (attn_heads)")
    g.add_argument("--config", type=str, default="./config.JSON")
    n = sub.add_parser("outliers", help="outlier identification: per interaction of a text file, its probability and its least supported loci")
    n.add_argument("-i", "--file", type=str, required=True)
    n.add_argument("-o", "--output", type=str, default="./outliers.tsv")
    n.add_argument("--lowest", type=int, default=3, help="loci to list per interaction, least supported first (0 .. 32)")
    n.add_argument("--scores", type=str, default=None, help="also write every locus's score to this .npz (sizes, offsets, scores)")
    n.add_argument("--config", type=str, default="./config.JSON")
    d.add_argument("--config", type=str, default="./config.JSON")
    for q in (a, b, c, e):
        q.add_argument("--config", type=str, default="./config.JSON")
    args = ap.parse_args(argv)
    config, temp_dir, model = _load(args.config)
    if args.cmd == "kway":
        return _kway(args, config, temp_dir, model)
    if args.cmd == "anchored":
        return _anchored(args, config, temp_dir, model)
    if args.cmd == "complete":
        return _complete(args, config, temp_dir, model)
    if args.cmd == "grow":
        return _grow(args, config, temp_dir, model)
    if args.cmd == "decompose":
        return _decompose(args, config, temp_dir, model)
    if args.cmd == "regions":
        return _regions(args, config, temp_dir, model)
    if args.cmd == "kmap":
        return _kmap(args, config, temp_dir, model)
    if args.cmd == "outliers":
        return _outliers(args, config, temp_dir, model)
    if args.cmd == "attention":
        bin2node = np.load(os.path.join(temp_dir, "bin2node.npy"), allow_pickle=True).item()
        samples = parse_file(args.file, bin2node, config["chrom_list"], config["resolution"], max_size=_lib.MAX_LONG_L)
        np.savez(args.output, **attention_maps(model, samples, per_head=args.per_head))
        print("%d interactions -> %s" % (len(samples), args.output))
        return
    if args.cmd == "multiway":
        bin2node = np.load(os.path.join(temp_dir, "bin2node.npy"), allow_pickle=True).item()
        samples, proba = predict_multiway(model, args.file, bin2node, config["chrom_list"], config["resolution"], args.output)
        print("%d interactions -> %s" % (len(samples), args.output))
    else:
        chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"))
        pairs, proba = pairwise_probabilities(model, chrom_range, args.chrom, config["min_distance"], task_mode=args.task_mode)
        np.save(args.output, proba2matrix(pairs, None, proba).cpu().numpy())
        print("%d pairs -> %s" % (len(pairs), args.output))


if __name__ == "__main__":
    main()
