"""De novo k-way sweep: which multi-way interactions, among ALL that could exist in a region, the trained
classifier believes in.

``predict multiway`` scores rows somebody wrote down and ``predict pairwise`` lists every pair; at k >= 3 the candidates of a
chromosome can neither be listed on the host nor their scores kept (chr1 at 1 Mb: 2.6 M triples, 159 M quadruples, 7.8 G
quintuples).  Here the candidates are made on the device from their rank, scored by ``model(x)`` chunk by chunk, and only the
best K (logit, rank) pairs are kept, on the device (csrc/sweep.hip).

A candidate of size k in the region [lo, lo + n) is a strictly ascending k-tuple of node ids whose adjacent differences are all
>= min_gap (min_gap = min_distance + 1: generate_kmers.py:18, :33 and the sampler).  Candidates are ordered lexicographically; the
rank of one is its position, from 0.  With m = n - (k - 1)(min_gap - 1), y_j = x_j - lo - j (min_gap - 1) maps them, order
preserved, onto the k-subsets of [0, m): C(m, k) candidates.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib


def _check_args(n: int, k: int, min_gap: int):
    if not (n >= 1 and 2 <= k <= _lib.MAX_L and min_gap >= 1):
        raise ValueError(f"need n >= 1, 2 <= k <= {_lib.MAX_L}, min_gap >= 1 (n={n} k={k} min_gap={min_gap})")


def kway_count(n: int, k: int, min_gap: int) -> int:
    """Number of candidates, C(n - (k - 1)(min_gap - 1), k); a count >= 2^63 is refused (ValueError), not truncated."""
    n, k, min_gap = int(n), int(k), int(min_gap)
    _check_args(n, k, min_gap)
    m = n - (k - 1) * (min_gap - 1)
    total = math.comb(m, k) if m >= k else 0
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (n={n} k={k} min_gap={min_gap}) do not fit 63 bits")
    return total


def kway_unrank(rank: int, lo: int, n: int, k: int, min_gap: int) -> Tuple[int, ...]:
    """The candidate of one rank, in Python integers (no GPU): how a rank is decoded, and the checker of the kernel."""
    total = kway_count(n, k, min_gap)
    rank = int(rank)
    if not 0 <= rank < total:
        raise IndexError(f"rank {rank} outside [0, {total})")
    m = n - (k - 1) * (min_gap - 1)
    # the lexicographic rank of y is total - 1 - (colexicographic rank of the mirrored set z_j = m - 1 - y_j): read z off the
    # combinatorial number system of q, largest element first
    row, q, upper = [], total - 1 - rank, m - 1
    for j in range(k, 0, -1):
        a, b = j - 1, upper                            # the largest c in [j - 1, upper] with C(c, j) <= q
        while a < b:
            mid = (a + b + 1) // 2
            if math.comb(mid, j) <= q:
                a = mid
            else:
                b = mid - 1
        q -= math.comb(a, j)
        row.append(int(lo) + (m - 1 - a) + (k - j) * (min_gap - 1))
        upper = a - 1
    return tuple(row)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def kway_rows(lo: int, n: int, k: int, min_gap: int, rank0: int = 0, count: Optional[int] = None, ranks: Optional[torch.Tensor] = None,
              width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [count, width] on the device: the candidates of ranks rank0 .. rank0 + count - 1, or of the device list ``ranks``
    (a rank outside [0, total) gives an all-zero row).  Columns k .. width - 1 are zero; ``out`` reuses a buffer of at least
    count * width elements."""
    lib = _lib.load()
    total = kway_count(n, k, min_gap)
    width = int(k if width is None else width)
    if not k <= width <= _lib.MAX_L:
        raise ValueError(f"width must be in [k, {_lib.MAX_L}]")
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        count, device = int(ranks.numel()), ranks.device
    else:
        count = total - int(rank0) if count is None else int(count)
        if rank0 < 0 or count < 0 or rank0 + count > total:
            raise IndexError(f"ranks [{rank0}, {rank0 + count}) outside [0, {total})")
    if out is None:
        x = torch.empty(count, width, dtype=torch.long, device=device)
    else:
        if out.dtype != torch.long or not out.is_contiguous() or out.numel() < count * width:
            raise ValueError("out must be a contiguous int64 tensor of at least count * width elements")
        x = out.view(-1)[:count * width].view(count, width)
    if not x.is_cuda:
        raise _lib.MatchaHipError("kway_rows needs a cuda device (no CPU fallback)")
    with torch.cuda.device(x.device):
        _lib.check(lib.matcha_kway_rows(int(lo), n, k, min_gap, int(rank0), _lib.ptr(ranks), count, width, _lib.ptr(x), _stream(x.device)),
                   "matcha_kway_rows")
    return x


class TopK:
    """Streaming selection on the device: after any sequence of ``update`` calls, ``result()`` is the best min(K, valid rows seen)
    (score, rank) pairs -- higher score first (IEEE comparison), then lower rank; NaN scores and skipped rows are never kept --
    bit for bit the same however the rows were cut into updates."""

    def __init__(self, K: int, max_chunk: int, device="cuda"):
        lib = _lib.load()
        self.K, self.max_chunk = int(K), int(max_chunk)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("TopK needs a cuda device (no CPU fallback)")
        self.bytes = int(lib.matcha_topk_bytes(self.K, self.max_chunk)) if 1 <= self.K < 1 << 31 else 0
        if self.bytes == 0:
            raise ValueError(f"TopK: need 1 <= K < 2^31 and 1 <= max_chunk < 2^31 (K={K} max_chunk={max_chunk})")
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_topk_init(_lib.ptr(self.state), self.bytes, self.K, self.max_chunk, _stream(self.device)), "matcha_topk_init")

    def update(self, scores: torch.Tensor, rank0: int, skip: Optional[torch.Tensor] = None):
        """``scores`` float32 [n] on the device (n <= max_chunk), row i of rank rank0 + i; ``skip`` int32 / bool [n], non-zero = never
        keep.  Enqueued on the current stream; nothing is read back."""
        lib = _lib.load()
        scores = scores.reshape(-1)
        if scores.dtype != torch.float32 or scores.device != self.state.device:
            raise ValueError("scores must be a float32 tensor on the TopK's device")
        scores = scores.contiguous()
        if skip is not None:
            skip = skip.reshape(-1).to(device=scores.device, dtype=torch.int32).contiguous()
            if skip.numel() != scores.numel():
                raise ValueError("skip and scores differ in length")
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_topk_update(_lib.ptr(self.state), self.bytes, self.K, self.max_chunk, _lib.ptr(scores), _lib.ptr(skip),
                                              scores.numel(), int(rank0), _stream(self.device)), "matcha_topk_update")

    def read(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(scores [K], ranks [K], n [1]) on the device, without a synchronisation; entries from n on are (0, -1)."""
        lib = _lib.load()
        scores = torch.empty(self.K, dtype=torch.float32, device=self.device)
        ranks = torch.empty(self.K, dtype=torch.long, device=self.device)
        n = torch.empty(1, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_topk_read(_lib.ptr(self.state), self.bytes, self.K, self.max_chunk, _lib.ptr(scores), _lib.ptr(ranks),
                                            _lib.ptr(n), _stream(self.device)), "matcha_topk_read")
        return scores, ranks, n

    def result(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores [K'], ranks [K']), best first, K' = min(K, valid rows seen): one synchronising read of K'."""
        scores, ranks, n = self.read()
        kept = int(n.item())
        return scores[:kept], ranks[:kept]


def kway_sweep(model, lo: int, hi: int, k: int, min_gap: int, top: int, chunk_rows: int = 1 << 20, width: Optional[int] = None,
               exclude=None, task_mode: str = "class") -> dict:
    """Score every candidate of size k in the region [lo, hi) of node ids and keep the ``top`` best.

    Returns ``rows`` int64 [K', width], ``logit`` [K'], ``proba`` [K'] (sigmoid of the logit, softplus for task_mode 'regress', as
    in pairwise_probabilities), ``rank`` int64 [K'] (decode one with kway_unrank), all on the model's device and best first, and
    the integers ``n_candidates`` and ``n_excluded``.  Selection is on the logits: the sigmoid saturates into ties, and the logit
    order is the probability order.  ``width`` (default k) zero-pads the rows: a row's logit depends on its batch's width because
    pads are attended, so ask for the width the other predictions used.  ``exclude``: a HyperedgeSet of known hyperedges; its
    members are skipped and counted, which is what makes the result de novo.

    Eval mode, no grad; per chunk: rows into one reused buffer, model(x), TopK.update -- nothing is copied to the host and nothing
    synchronises until the end, where the node-id check of the whole sweep is raised once (IndexError for a region beyond the
    model's tables) and the winners' rows are made from their ranks."""
    if task_mode not in ("class", "regress"):
        raise ValueError("task_mode must be 'class' or 'regress'")
    lo, hi, k, min_gap, top, chunk_rows = int(lo), int(hi), int(k), int(min_gap), int(top), int(chunk_rows)
    n = hi - lo
    width = int(k if width is None else width)
    if not k <= width <= _lib.MAX_L:
        raise ValueError(f"width must be in [k, {_lib.MAX_L}]")
    if top < 1 or chunk_rows < 1:
        raise ValueError("top and chunk_rows must be >= 1")
    act = torch.nn.functional.softplus if task_mode == "regress" else torch.sigmoid
    model.eval()
    dev = model.layer_norm1.weight.device
    total = kway_count(n, k, min_gap) if n >= 1 else 0
    if total == 0:
        e = torch.empty(0, dtype=torch.float32, device=dev)
        return {"rows": torch.empty(0, width, dtype=torch.long, device=dev), "logit": e, "proba": e.clone(),
                "rank": torch.empty(0, dtype=torch.long, device=dev), "n_candidates": 0, "n_excluded": 0}
    chunk_rows = min(chunk_rows, total)
    sel = TopK(min(top, total), chunk_rows, dev)
    buf = torch.empty(chunk_rows * width, dtype=torch.long, device=dev)
    n_exc = torch.zeros((), dtype=torch.long, device=dev)
    # The library picks its forward kernels by batch size (csrc/fused_fwd32.hip: up to two half tiles per compute unit go to the
    # small-batch kernels), and the two routes round differently (a few ulp of the logit).  The sweep pins the large-batch route, so
    # a candidate's logit does not depend on chunk_rows, on the size of the region or on the last chunk being short.
    with torch.no_grad(), model.deferred_id_check(), _lib.option("disable_small_batch"):
        for r0 in range(0, total, chunk_rows):
            x = kway_rows(lo, n, k, min_gap, rank0=r0, count=min(chunk_rows, total - r0), width=width, out=buf)
            logits = model(x).reshape(-1)
            skip = None
            if exclude is not None:
                skip = exclude.contains(x)
                n_exc += skip.sum()
            sel.update(logits, r0, skip)
    logit, rank = sel.result()
    rows = kway_rows(lo, n, k, min_gap, ranks=rank, width=width, device=dev)
    return {"rows": rows, "logit": logit, "proba": act(logit), "rank": rank, "n_candidates": total, "n_excluded": int(n_exc.item())}
