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

``anchored_sweep`` keeps the best K per anchor instead of one global list; ``kway_map`` / ``PairMap`` (DESIGN.md 7.5,
csrc/pairmap.hip) project the scores of all candidates onto pairs of bins instead of keeping a list at all.  ``completion_sweep``
 extends clusters of 1 to 31 loci by bins of a region; ``decomposition_sweep`` ranks the sub-hyperedges
made of a cluster's own loci, or the cluster with some of them taken out, and sums the scores per locus (``SubsetSupport``).
``growth_sweep`` (csrc/grow.hip) beam-searches hubs of up to 32 loci from seed clusters, one bin per step (``grow_step``).
``region_sweep`` / ``region_map`` draw a candidate's bins from up to 8 ascending, disjoint regions -- one bin on chr1, one on
chr6, two on chr11: each part contributes one candidate of its own region, the global rank is the mixed radix of the parts' ranks
(``region_count``, ``region_unrank``, ``region_rows``), and the result is the best K overall, the best K per candidate of the leading part, or
the pair map between two parts.

The loop.  Every driver here and in matcha_amd/expected.py walks its candidates through ``_chunks`` under ``_pinned``.  ``_pinned(model)`` holds
no_grad, the model's deferred node-id check (raised once, when the block ends: IndexError) and the large-batch forward route, so a logit does
not depend on the cut.  ``_chunks`` cuts ``total`` ranks into chunks of min(chunk_rows, total); per chunk it has ``rows(g0, count, buf, fbuf)``
fill the reused buffers (x, or x and a flag per row), scores x with model(x) (or ``forward(g0, x)``), and settles ``skip``: flag != 0, or a
member of ``exclude``; None when the source has no flags and there is no ``exclude``, so the sink gets a null pointer.  ``n_invalid`` counts
the flagged rows and ``n_excluded`` the members of ``exclude`` that are not flagged, as device scalars in ``tally``.  It yields (g0, x, logits,
skip, flag) to the driver, whose body holds only its own sinks.  Nothing is copied to the host and nothing synchronises per chunk; an empty
sweep returns before anything is allocated or launched.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
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


def _free_count(n: int, f: int, min_gap: int) -> int:
    """C_f: the gap-constrained subsets of size f >= 1 of a region of n nodes (f = 1: n)."""
    m = n - (f - 1) * (min_gap - 1)
    return math.comb(m, f) if m >= f else 0


def _subset_unrank(rank: int, lo: int, n: int, f: int, min_gap: int) -> Tuple[int, ...]:
    """The gap-constrained subset of size f >= 1 of [lo, lo + n) of lexicographic rank ``rank``, 0 <= rank < C_f, in Python integers:
    the one decoder behind every *_unrank here."""
    m = n - (f - 1) * (min_gap - 1)
    # the lexicographic rank of y is total - 1 - (colexicographic rank of the mirrored set z_j = m - 1 - y_j): read z off the
    # combinatorial number system of q, largest element first
    row, q, upper = [], _free_count(n, f, min_gap) - 1 - rank, m - 1
    for j in range(f, 0, -1):
        a, b = j - 1, upper                            # the largest c in [j - 1, upper] with C(c, j) <= q
        while a < b:
            mid = (a + b + 1) // 2
            if math.comb(mid, j) <= q:
                a = mid
            else:
                b = mid - 1
        q -= math.comb(a, j)
        row.append(lo + (m - 1 - a) + (f - j) * (min_gap - 1))
        upper = a - 1
    return tuple(row)


def _checked_rank(rank: int, total: int) -> int:
    rank = int(rank)
    if not 0 <= rank < total:
        raise IndexError(f"rank {rank} outside [0, {total})")
    return rank


def kway_unrank(rank: int, lo: int, n: int, k: int, min_gap: int) -> Tuple[int, ...]:
    """The candidate of one rank, in Python integers (no GPU): how a rank is decoded, and the checker of the kernel."""
    rank = _checked_rank(rank, kway_count(n, k, min_gap))
    return _subset_unrank(rank, int(lo), int(n), int(k), int(min_gap))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _activation(task_mode: str):
    """What turns a logit into the value reported: sigmoid, softplus for task_mode 'regress' (as in pairwise_probabilities)."""
    if task_mode not in ("class", "regress"):
        raise ValueError("task_mode must be 'class' or 'regress'")
    return torch.nn.functional.softplus if task_mode == "regress" else torch.sigmoid


def _check_width(k: int, width: Optional[int]) -> int:
    width = int(k if width is None else width)
    if not k <= width <= _lib.MAX_L:
        raise ValueError(f"width must be in [k, {_lib.MAX_L}]")
    return width


def _check_sweep_args(k: int, width: Optional[int], chunk_rows: int, top: int = 1) -> int:
    """The width of a sweep of rows of up to 8 columns (default k), once ``top`` and ``chunk_rows`` are known to be usable."""
    width = _check_width(k, width)
    if top < 1 or chunk_rows < 1:
        raise ValueError("top and chunk_rows must be >= 1")
    return width


def _rank_range(total: int, rank0: int, count: Optional[int], ranks: Optional[torch.Tensor]) -> int:
    """How many rows a rows call makes: the length of the list ``ranks`` (``rank0`` is not looked at), or ``count`` (default: everything
    from ``rank0`` on); a range that leaves [0, total) is an IndexError."""
    if ranks is not None:
        return int(ranks.numel())
    rank0 = int(rank0)
    count = total - rank0 if count is None else int(count)
    if rank0 < 0 or count < 0 or rank0 + count > total:
        raise IndexError(f"ranks [{rank0}, {rank0 + count}) outside [0, {total})")
    return count


def _row_buffers(count: int, width: int, device, out: Optional[torch.Tensor], flag_out: Optional[torch.Tensor], who: str, flags: bool = True):
    """(x int64 [count, width], flag int32 [count]) on ``device``: fresh, or the leading elements of ``out`` / ``flag_out`` once they are
    seen to be contiguous, of the right type, large enough and on that device.  ``flags=False``: no flag, (x, None)."""
    if out is None:
        x = torch.empty(count, width, dtype=torch.long, device=device)
    else:
        if out.dtype != torch.long or not out.is_contiguous() or out.numel() < count * width or out.device != device:
            raise ValueError(f"{who}: out must be a contiguous int64 tensor of at least count * width elements on the rows' device")
        x = out.view(-1)[:count * width].view(count, width)
    if not flags:
        return x, None
    if flag_out is None:
        flag = torch.empty(count, dtype=torch.int32, device=device)
    else:
        if flag_out.dtype != torch.int32 or not flag_out.is_contiguous() or flag_out.numel() < count or flag_out.device != x.device:
            raise ValueError(f"{who}: flag_out must be a contiguous int32 tensor of at least count elements on out's device")
        flag = flag_out.view(-1)[:count]
    return x, flag


def _scores_and_skip(scores: torch.Tensor, skip: Optional[torch.Tensor], device, who: str):
    """What every sink's ``update`` takes: (float32 [n] contiguous on ``device``, int32 [n] or None)."""
    scores = scores.reshape(-1)
    if scores.dtype != torch.float32 or scores.device != device:
        raise ValueError(f"scores (values) must be a float32 tensor on the {who}'s device")
    scores = scores.contiguous()
    if skip is not None:
        skip = skip.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
        if skip.numel() != scores.numel():
            raise ValueError("skip and scores (values) differ in length")
    return scores, skip


# ---- the loop (see the module's docstring) -------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _pinned(model):
    """no_grad, the node-id check of everything inside raised once at the end (IndexError), and ONE forward route.

    The library picks its forward kernels by batch size (csrc/fused_fwd32.hip: up to two half tiles per compute unit go to the
    small-batch kernels), and the two routes round differently (a few ulp of the logit).  A sweep pins the large-batch route, so a
    candidate's logit does not depend on chunk_rows, on the size of the region or on the last chunk being short.  Beyond 8 columns
    the long forward has one route: its kernels are chosen by the model's shape, never by the batch, and every token row is computed
    by itself, so a logit does not depend on chunk_rows there either."""
    with torch.no_grad(), model.deferred_id_check(), _lib.option("disable_small_batch"):
        yield


def _buffers(most_rows: int, width: int, device, flags: bool = True):
    """The loop's reused (row buffer, flag buffer or None) for chunks of up to ``most_rows`` rows."""
    return (torch.empty(most_rows * width, dtype=torch.long, device=device),
            torch.empty(most_rows, dtype=torch.int32, device=device) if flags else None)


def _tally(device, *names) -> dict:
    """Zeroed device scalars, the loop's counters ('n_invalid', 'n_excluded'); ``_counted`` reads them back."""
    return {name: torch.zeros((), dtype=torch.long, device=device) for name in names}


def _counted(tally: dict) -> dict:
    return {name: int(t.item()) for name, t in tally.items()}


def _chunks(model, total: int, chunk_rows: int, buffers, rows, exclude, tally: dict, forward=None):
    """Walk the ranks [0, total) in chunks of min(chunk_rows, total) and yield (g0, x, logits, skip, flag) per chunk.

    ``rows(g0, count, buf, fbuf)`` makes the candidates of the ranks g0 .. g0 + count - 1 in ``buffers`` = (buf, fbuf) (``_buffers``; they
    may serve several walks) and returns x, or (x, flag) with flag != 0 for an invalid candidate; ``flag`` is yielded as None for a source
    without flags.  ``logits`` = model(x).reshape(-1), or ``forward(g0, x)`` where something else stands in for it (a cache of logits, a
    map's values).  ``skip``: flagged or in ``exclude`` (an object with ``contains(x)``); None without flags and without ``exclude``.
    ``tally['n_invalid']`` (where present) counts the flagged rows, ``tally['n_excluded']`` the members of ``exclude`` not flagged."""
    chunk = min(chunk_rows, total)
    buf, fbuf = buffers
    n_inv = tally.get("n_invalid")
    for g0 in range(0, total, chunk):
        made = rows(g0, min(chunk, total - g0), buf, fbuf)
        x, flag = made if isinstance(made, tuple) else (made, None)
        logits = model(x).reshape(-1) if forward is None else forward(g0, x)
        skip = None
        if flag is not None:
            skip = flag != 0
            if n_inv is not None:
                n_inv += skip.sum()
        if exclude is not None:
            known = exclude.contains(x)
            if skip is None:
                tally["n_excluded"] += known.sum()
                skip = known
            else:
                tally["n_excluded"] += (known & ~skip).sum()
                skip = skip | known
        yield g0, x, logits, skip, flag


def _long_chunk_rows(model, chunk_rows: Optional[int], width: int) -> int:
    """The chunk of a sweep whose rows may be long.  None: 2^20 rows up to width 8 and min(2^20, 2^21 // width) beyond (about 3.1 KB of
    workspace per token); an explicit value the long forward cannot take is a ValueError before anything is launched."""
    if chunk_rows is None:
        return 1 << 20 if width <= _lib.MAX_L else min(1 << 20, (1 << 21) // width)
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1")
    if width > _lib.MAX_L:
        rt = model._runtime()
        if not chunk_rows < 1 << 31 or rt.lib.matcha_workspace_bytes_long(C.byref(rt.shape), chunk_rows, width) == 0:
            raise ValueError(f"chunk_rows = {chunk_rows} rows of {width} columns are more than the long forward takes in one call")
    return chunk_rows


def _per_segment(grank: torch.Tensor, logit: torch.Tensor, seg_len: int, act):
    """(rank within its segment, proba) [A, K] of a SegTopK's read: segment a holds the global ranks from a * seg_len on; where nothing
    was kept the rank stays -1 and proba is 0."""
    kept = grank >= 0
    first = torch.arange(grank.shape[0], dtype=torch.long, device=grank.device).view(-1, 1) * seg_len
    return torch.where(kept, grank - first, grank), torch.where(kept, act(logit), torch.zeros_like(logit))


def _empty_segments(A: int, K: int, width: int, dev) -> dict:
    """The per-segment keys with nothing kept: rank -1, everything else 0."""
    e = torch.zeros(A, K, dtype=torch.float32, device=dev)
    return {"rows": torch.zeros(A, K, width, dtype=torch.long, device=dev), "logit": e, "proba": e.clone(),
            "rank": torch.full((A, K), -1, dtype=torch.long, device=dev), "count": torch.zeros(A, dtype=torch.long, device=dev)}


def kway_rows(lo: int, n: int, k: int, min_gap: int, rank0: int = 0, count: Optional[int] = None, ranks: Optional[torch.Tensor] = None,
              width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [count, width] on the device: the candidates of ranks rank0 .. rank0 + count - 1, or of the device list ``ranks``
    (a rank outside [0, total) gives an all-zero row).  Columns k .. width - 1 are zero (k <= width <= 8); ``out`` reuses a buffer of at least
    count * width elements."""
    lib = _lib.load()
    total = kway_count(n, k, min_gap)
    width = _check_width(k, width)
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        device = ranks.device
    count = _rank_range(total, rank0, count, ranks)
    x, _ = _row_buffers(count, width, device if out is None else out.device, out, None, "kway_rows", flags=False)
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
        scores, skip = _scores_and_skip(scores, skip, self.state.device, "TopK")
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
    pads are attended, so ask for the width the other predictions used (k and width stay at most 8 here: the long forward of model(x), 9 .. 32 columns, has no sweep).  ``exclude``: a HyperedgeSet of known hyperedges; its
    members are skipped and counted, which is what makes the result de novo.

    Eval mode and the loop (see the module's docstring) with kway_rows and TopK.update: nothing synchronises until the end, where the
    node-id check of the whole sweep is raised once (IndexError for a region beyond the model's tables) and the winners' rows are made
    from their ranks."""
    act = _activation(task_mode)
    lo, hi, k, min_gap, top, chunk_rows = int(lo), int(hi), int(k), int(min_gap), int(top), int(chunk_rows)
    n = hi - lo
    width = _check_sweep_args(k, width, chunk_rows, top)
    model.eval()
    dev = model.layer_norm1.weight.device
    total = kway_count(n, k, min_gap) if n >= 1 else 0
    if total == 0:
        e = torch.empty(0, dtype=torch.float32, device=dev)
        return {"rows": torch.empty(0, width, dtype=torch.long, device=dev), "logit": e, "proba": e.clone(),
                "rank": torch.empty(0, dtype=torch.long, device=dev), "n_candidates": 0, "n_excluded": 0}
    chunk_rows = min(chunk_rows, total)
    sel = TopK(min(top, total), chunk_rows, dev)
    tally = _tally(dev, "n_excluded")
    rows = lambda r0, count, buf, _: kway_rows(lo, n, k, min_gap, rank0=r0, count=count, width=width, out=buf)
    with _pinned(model):
        for r0, _, logits, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev, flags=False), rows, exclude, tally):
            sel.update(logits, r0, skip)
    logit, rank = sel.result()
    rows = kway_rows(lo, n, k, min_gap, ranks=rank, width=width, device=dev)
    return {"rows": rows, "logit": logit, "proba": act(logit), "rank": rank, "n_candidates": total, **_counted(tally)}


# ---- anchored sweep: the best K completions of every anchor -------------------------------------------------------
def _check_anchor_args(A: int, s: int, n: int, k: int, min_gap: int):
    if not (A >= 0 and n >= 1 and 2 <= k <= _lib.MAX_L and 1 <= s <= k - 1 and min_gap >= 1):
        raise ValueError(f"need A >= 0, n >= 1, 2 <= k <= {_lib.MAX_L}, 1 <= s <= k - 1, min_gap >= 1 (A={A} s={s} n={n} k={k} min_gap={min_gap})")


def anchored_count(A: int, s: int, n: int, k: int, min_gap: int) -> int:
    """Number of global ranks, A * C_f with C_f = C(n - (f - 1)(min_gap - 1), f) and f = k - s free nodes per candidate; a total
    >= 2^63 is refused (ValueError), not truncated."""
    A, s, n, k, min_gap = int(A), int(s), int(n), int(k), int(min_gap)
    _check_anchor_args(A, s, n, k, min_gap)
    total = A * _free_count(n, k - s, min_gap)
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (A={A} s={s} n={n} k={k} min_gap={min_gap}) do not fit 63 bits")
    return total


def anchored_unrank(rank: int, anchor_row, lo: int, n: int, k: int, min_gap: int) -> Tuple[Tuple[int, ...], bool]:
    """(row, valid) of one anchor's candidate of FREE rank ``rank`` (a global rank g is anchor g // C_f, free rank g % C_f), in
    Python integers (no GPU).  The row is the anchor's ids and the free part -- the gap-constrained subset of size k - s of
    [lo, lo + n) of that lexicographic rank -- sorted ascending, duplicates kept; it is valid iff every adjacent difference is
    >= min_gap."""
    anchor_row = [int(v) for v in anchor_row]
    s, lo, n, k, min_gap = len(anchor_row), int(lo), int(n), int(k), int(min_gap)
    _check_anchor_args(1, s, n, k, min_gap)
    rank = _checked_rank(rank, _free_count(n, k - s, min_gap))
    row = tuple(sorted(anchor_row + list(_subset_unrank(rank, lo, n, k - s, min_gap))))
    return row, all(b - a >= min_gap for a, b in zip(row, row[1:]))


def _anchor_table(anchors, device) -> torch.Tensor:
    """int64 [A, s] on the device; a 1-D input is A single anchors."""
    t = torch.as_tensor(anchors)
    if t.dim() == 1:
        t = t.view(-1, 1)
    if t.dim() != 2 or t.is_floating_point():
        raise ValueError("anchors must be an integer [A, s] (or [A]) tensor or array")
    return t.to(device=device, dtype=torch.long).contiguous()


def anchored_rows(anchors, lo: int, n: int, k: int, min_gap: int, rank0: int = 0, count: Optional[int] = None,
                  ranks: Optional[torch.Tensor] = None, width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None,
                  flag_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x int64 [count, width], flag int32 [count]) on the device: the candidates of the global ranks rank0 .. rank0 + count - 1, or
    of the device list ``ranks`` (a rank outside [0, A * C_f) gives an all-zero row with its flag set); flag != 0 marks an invalid
    candidate.  ``anchors``: int64 [A, s] (a device tensor is used as it is).  ``out`` / ``flag_out`` reuse buffers of at least
    count * width / count elements."""
    lib = _lib.load()
    if isinstance(anchors, torch.Tensor) and anchors.is_cuda and ranks is None and out is None:
        device = anchors.device
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        device = ranks.device
    elif out is not None:
        device = out.device
    anchors = _anchor_table(anchors, device)
    A, s = int(anchors.shape[0]), int(anchors.shape[1])
    total = anchored_count(A, s, n, k, min_gap)
    width = _check_width(k, width)
    count = _rank_range(total, rank0, count, ranks)
    x, flag = _row_buffers(count, width, anchors.device, out, flag_out, "anchored_rows")
    if not x.is_cuda:
        raise _lib.MatchaHipError("anchored_rows needs a cuda device (no CPU fallback)")
    with torch.cuda.device(x.device):
        _lib.check(lib.matcha_kway_anchor_rows(_lib.ptr(anchors), A, s, int(lo), n, k, min_gap, int(rank0), _lib.ptr(ranks), count, width,
                                               _lib.ptr(x), _lib.ptr(flag), _stream(x.device)), "matcha_kway_anchor_rows")
    return x, flag


class SegTopK:
    """One streaming top-K per segment, on the device: the state covers ``A`` segments of ``seg_len`` consecutive global ranks
    starting at segment ``first_segment``; after any sequence of ``update`` calls segment a holds its best min(K, valid rows seen)
    (score, global rank) pairs in TopK's order -- bit for bit the same however the rows were cut into updates.  A chunk may begin
    and end inside a segment and cover a fraction of one or thousands of them; segments it does not touch are left alone."""

    def __init__(self, A: int, K: int, seg_len: int, max_chunk: int, device="cuda", first_segment: int = 0):
        lib = _lib.load()
        self.A, self.K, self.seg_len, self.max_chunk, self.first_segment = int(A), int(K), int(seg_len), int(max_chunk), int(first_segment)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("SegTopK needs a cuda device (no CPU fallback)")
        fits = 1 <= self.K < 1 << 31 and 1 <= self.A < 1 << 31 and 1 <= self.seg_len < 1 << 63 and 1 <= self.max_chunk < 1 << 31
        self.bytes = int(lib.matcha_segtopk_bytes(self.A, self.K, self.seg_len, self.max_chunk)) if fits else 0
        if self.bytes == 0 or not 0 <= self.first_segment < 1 << 62:
            raise ValueError(f"SegTopK: need 1 <= K, 1 <= A, A * K < 2^31, seg_len >= 1 and 1 <= max_chunk < 2^31 "
                             f"(A={A} K={K} seg_len={seg_len} max_chunk={max_chunk})")
        self._dims = (self.A, self.K, self.seg_len, self.max_chunk)
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_segtopk_init(_lib.ptr(self.state), self.bytes, *self._dims, _stream(self.device)), "matcha_segtopk_init")

    def update(self, scores: torch.Tensor, g0: int, skip: Optional[torch.Tensor] = None):
        """``scores`` float32 [n] on the device (n <= max_chunk), row i of global rank g0 + i (segment (g0 + i) // seg_len);
        ``skip`` int32 / bool [n], non-zero = never keep.  Enqueued on the current stream; nothing is read back."""
        lib = _lib.load()
        scores, skip = _scores_and_skip(scores, skip, self.state.device, "SegTopK")
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_segtopk_update(_lib.ptr(self.state), self.bytes, *self._dims, self.first_segment, _lib.ptr(scores),
                                                 _lib.ptr(skip), scores.numel(), int(g0), _stream(self.device)), "matcha_segtopk_update")

    def read(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(scores [A, K], global ranks [A, K], counts [A]) on the device, without a synchronisation; best first within a segment,
        entries from counts[a] on are (0, -1)."""
        lib = _lib.load()
        scores = torch.empty(self.A, self.K, dtype=torch.float32, device=self.device)
        ranks = torch.empty(self.A, self.K, dtype=torch.long, device=self.device)
        counts = torch.empty(self.A, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_segtopk_read(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(scores), _lib.ptr(ranks),
                                               _lib.ptr(counts), _stream(self.device)), "matcha_segtopk_read")
        return scores, ranks, counts


def anchored_sweep(model, anchors, lo: int, hi: int, k: int, min_gap: int, top: int, chunk_rows: int = 1 << 20, width: Optional[int] = None,
                   exclude=None, task_mode: str = "class") -> dict:
    """For every anchor row (``anchors`` int64 [A, s], 1-D = single anchors, 1 <= s <= k - 1) score all its completions by a
    gap-constrained subset of size k - s of the partner region [lo, hi) and keep the ``top`` best PER ANCHOR.  Anchors may lie inside
    the region, outside it or on another chromosome; the gap rule is on node-id differences only.

    Returns, on the model's device and best first within each anchor, with K = min(top, C_f): ``rows`` int64 [A, K, width],
    ``logit`` and ``proba`` [A, K], ``rank`` int64 [A, K] (the FREE rank; decode with anchored_unrank(rank, anchors[a], ...)) and
    ``count`` int64 [A]; beyond count[a] the rank is -1 and rows, logit and proba are 0.  The integers ``n_candidates`` = A * C_f,
    ``n_invalid`` (candidates that break the rule: a free node on or too near an anchor, or an anchor row that breaks it itself;
    they are scored but never kept) and ``n_excluded`` (valid candidates found in ``exclude``).

    Eval mode and the loop (see the module's docstring) with anchored_rows and SegTopK.update: nothing synchronises until the end,
    where the node-id check of the whole sweep is raised once (IndexError, also for an anchor beyond the model's tables)."""
    act = _activation(task_mode)
    lo, hi, k, min_gap, top, chunk_rows = int(lo), int(hi), int(k), int(min_gap), int(top), int(chunk_rows)
    n = hi - lo
    width = _check_sweep_args(k, width, chunk_rows, top)
    model.eval()
    dev = model.layer_norm1.weight.device
    anchors = _anchor_table(anchors, dev)
    A, s = int(anchors.shape[0]), int(anchors.shape[1])
    total = anchored_count(A, s, n, k, min_gap) if n >= 1 else 0
    cf = total // A if A else 0
    K = min(top, cf)
    if total == 0:
        return {**_empty_segments(A, K, width, dev), "n_candidates": 0, "n_invalid": 0, "n_excluded": 0}
    chunk_rows = min(chunk_rows, total)
    sel = SegTopK(A, K, cf, chunk_rows, dev)
    tally = _tally(dev, "n_invalid", "n_excluded")
    rows = lambda g0, count, buf, fbuf: anchored_rows(anchors, lo, n, k, min_gap, rank0=g0, count=count, width=width, out=buf, flag_out=fbuf)
    with _pinned(model):
        for g0, _, logits, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev), rows, exclude, tally):
            sel.update(logits, g0, skip)
    logit, grank, count = sel.read()
    rows, _ = anchored_rows(anchors, lo, n, k, min_gap, ranks=grank, width=width, device=dev)
    rank, proba = _per_segment(grank, logit, cf, act)
    return {"rows": rows.view(A, K, width), "logit": logit, "proba": proba, "rank": rank, "count": count, "n_candidates": total,
            **_counted(tally)}


# ---- pair maps: a sweep's scores projected onto pairs of bins ------------------------------------------------------
_PLANE_ORDER = ("sum", "count", "count_ge", "max")


def _plane_mask(planes) -> int:
    if planes is None or planes == "all":
        return _lib.PAIRMAP_ALL
    if isinstance(planes, int):
        mask = int(planes)
    else:
        names = [planes] if isinstance(planes, str) else list(planes)
        unknown = [p for p in names if p not in _lib.PAIRMAP_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose among {_PLANE_ORDER}")
        mask = sum(_lib.PAIRMAP_PLANES[p] for p in set(names))
    if not 1 <= mask <= _lib.PAIRMAP_ALL:
        raise ValueError(f"the plane mask must be in [1, {_lib.PAIRMAP_ALL}] (got {mask})")
    return mask


class PairMap:
    """Pair map on the device (csrc/pairmap.hip): ``rows`` = (lo, n) and ``cols`` = (lo, n) are two regions of node ids, equal
    (symmetric map) or disjoint (rectangular map).  Every accepted row of an ``update`` adds its value to the cell of each pair of its
    positions (see ``update``).  ``planes``: 'all', a bit mask, or names among 'sum', 'count', 'count_ge', 'max' -- only those take
    memory.  The sum is kept in fixed point (int64, 32 fractional bits) and everything is accumulated with integer atomics, so every
    plane is bit for bit the same whatever the order of the rows and however they were cut into updates.  ``vmax``: the largest value
    accepted, 0 < vmax <= 2^20; a cell's sum is exact while it stays below 2^31.  ``threshold``: what 'count_ge' counts (value >=
    threshold, in float32)."""

    def __init__(self, rows, cols, planes="all", vmax: float = 1.0, threshold: float = 0.5, device="cuda"):
        lib = _lib.load()
        (self.lo_r, self.n_r), (self.lo_c, self.n_c) = (int(rows[0]), int(rows[1])), (int(cols[0]), int(cols[1]))
        self.planes = _plane_mask(planes)
        self.vmax, self.threshold = float(vmax), float(threshold)
        self.symmetric = (self.lo_r, self.n_r) == (self.lo_c, self.n_c)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("PairMap needs a cuda device (no CPU fallback)")
        fits = all(0 <= lo < 1 << 62 for lo in (self.lo_r, self.lo_c)) and all(1 <= n < 1 << 31 for n in (self.n_r, self.n_c))
        self._dims = (self.lo_r, self.n_r, self.lo_c, self.n_c, self.planes, self.vmax, self.threshold)
        self.bytes = int(lib.matcha_pairmap_bytes(*self._dims)) if fits else 0
        if self.bytes == 0:
            raise ValueError(f"PairMap: need two regions (lo >= 0, n >= 1) that are equal or disjoint, n_r * n_c < 2^31 and 0 < vmax <= 2^20 "
                             f"(rows={rows} cols={cols} vmax={vmax})")
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_pairmap_init(_lib.ptr(self.state), self.bytes, *self._dims, _stream(self.device)), "matcha_pairmap_init")

    def update(self, x: torch.Tensor, value: torch.Tensor, skip: Optional[torch.Tensor] = None):
        """``x`` int64 [n, L] on the device (2 <= L <= 8, 0 = padding; rows need not be sorted), ``value`` float32 [n], ``skip``
        int32 / bool [n] (non-zero = the row contributes nothing; anchored_rows' flag and HyperedgeSet.contains fit).  A row whose
        value is NaN, negative or > vmax is counted as rejected and contributes nothing.  For each pair of positions ci < cj with
        ids a, b both non-zero and different: rectangular, cell (a - lo_r, b - lo_c) if a is a row id and b a column id, or the
        other way round; symmetric, the unordered pair.  Enqueued on the current stream; nothing is read back."""
        lib = _lib.load()
        if x.dim() != 2 or x.dtype != torch.long or x.device != self.state.device:
            raise ValueError("x must be an int64 [n, L] tensor on the PairMap's device")
        value, skip = _scores_and_skip(value, skip, self.state.device, "PairMap")
        if value.numel() != x.shape[0]:
            raise ValueError("value must hold one float32 per row of x")
        x = x.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_pairmap_update(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(x), _lib.ptr(value), _lib.ptr(skip),
                                                 int(x.shape[0]), int(x.shape[1]), _stream(self.device)), "matcha_pairmap_update")

    def read(self) -> dict:
        """The planes present as they are kept, on the device and without a synchronisation: 'sum' int64 [n_r, n_c] (fixed point,
        value * 2^32), 'count' and 'count_ge' int64, 'max' float32 (-inf where nothing landed); a symmetric map comes mirrored
        with a zero diagonal.  'counters' int64 [2] = (accepted rows, rejected rows)."""
        lib = _lib.load()
        out = {}
        counters = torch.empty(2, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            for name in _PLANE_ORDER:
                bit = _lib.PAIRMAP_PLANES[name]
                if not self.planes & bit:
                    continue
                t = torch.empty(self.n_r, self.n_c, dtype=torch.float32 if name == "max" else torch.long, device=self.device)
                _lib.check(lib.matcha_pairmap_read(_lib.ptr(self.state), self.bytes, *self._dims, bit, _lib.ptr(t), _lib.ptr(counters),
                                                   _stream(self.device)), "matcha_pairmap_read")
                out[name] = t
        out["counters"] = counters
        return out

    def result(self) -> dict:
        """The planes present, on the device: 'sum' float64 (the fixed-point sum / 2^32), 'count', 'count_ge', 'max', and -- when
        sum and count are both kept -- 'mean' float32 = sum / count (0 where count is 0); 'n_rows' and 'n_rejected' as 0-d int64
        tensors."""
        raw = self.read()
        counters = raw.pop("counters")
        out = dict(raw)
        if "sum" in out:
            out["sum"] = out["sum"].to(torch.float64) / 4294967296.0
        if "sum" in out and "count" in out:
            hit = out["count"] > 0
            out["mean"] = torch.where(hit, out["sum"] / out["count"].clamp(min=1).to(torch.float64), torch.zeros_like(out["sum"])).to(torch.float32)
        out["n_rows"], out["n_rejected"] = counters[0], counters[1]
        return out


def _empty_map(n_r: int, n_c: int, mask: int, dev) -> dict:
    out = {}
    if mask & _lib.PAIRMAP_SUM:
        out["sum"] = torch.zeros(n_r, n_c, dtype=torch.float64, device=dev)
    if mask & _lib.PAIRMAP_COUNT:
        out["count"] = torch.zeros(n_r, n_c, dtype=torch.long, device=dev)
    if mask & _lib.PAIRMAP_COUNT_GE:
        out["count_ge"] = torch.zeros(n_r, n_c, dtype=torch.long, device=dev)
    if mask & _lib.PAIRMAP_MAX:
        out["max"] = torch.full((n_r, n_c), float("-inf"), dtype=torch.float32, device=dev)
        if n_r == n_c:
            out["max"].fill_diagonal_(0.0)
    if "sum" in out and "count" in out:
        out["mean"] = torch.zeros(n_r, n_c, dtype=torch.float32, device=dev)
    return out


def kway_map(model, lo: int, hi: int, k: int, min_gap: int, chunk_rows: int = 1 << 20, width: Optional[int] = None, exclude=None,
             task_mode: str = "class", threshold: float = 0.5, planes="all", value_max: Optional[float] = None,
             row_window: Optional[Tuple[int, int]] = None, col_window: Optional[Tuple[int, int]] = None, expected=None, mode: str = "ratio",
             min_count: int = 30) -> dict:
    """Score every candidate of size k in the region [lo, hi) (kway_sweep's candidates, in its order, through the same loop) and project
    the probabilities onto pairs of bins: for every pair, the summed probability of the candidates that contain it ('sum', float64),
    their number ('count'), how many reach ``threshold`` ('count_ge'), the best of them ('max', -inf where there is none) and
    'mean' = sum / count -- the multi-way counterpart of the pairwise probability matrix.

    The default map is symmetric over [lo, hi) ([n, n], mirrored, zero diagonal).  ``row_window`` and ``col_window``, two disjoint
    (lo, n) windows inside the region, give the rectangular block [row bins, column bins] of the same map instead.  The value of a
    candidate is sigmoid(logit), or softplus(logit) for task_mode 'regress', where ``value_max`` (the largest value accepted, <= 2^20)
    is required: larger values, and NaN, are counted in ``n_rejected`` and contribute nothing.  The sum is exact in fixed point while
    a cell's total stays below 2^31; a sweep whose bound per cell, C(m, k - 2) * vmax with m = n - (k - 1)(min_gap - 1), reaches
    2^31 is refused before anything is launched.  ``exclude``, ``width`` and ``chunk_rows`` as in kway_sweep; the planes do not depend
    on ``chunk_rows``, bit for bit.

    ``expected`` (a GapExpected of matcha_amd/expected.py) gives the observed-over-expected map: a candidate's value is
    its activated value divided by the mean of its gap stratum (``mode`` 'ratio', the only one a map of non-negative values takes;
    ``min_count`` as in GapExpected.table), ``value_max`` defaults to 1024, and candidates of undersampled strata (their ratio is NaN)
    land in ``n_rejected`` with the ratios above ``value_max``.  Without ``expected`` nothing changes, bit for bit.

    Returns the planes (device tensors) and the integers ``n_candidates``, ``n_excluded`` and ``n_rejected``.  Nothing synchronises
    until the end, where the node-id check of the whole sweep is raised once (IndexError)."""
    act = _activation(task_mode)
    if expected is not None:
        if mode != "ratio":
            raise ValueError("kway_map accumulates non-negative values: with expected only mode 'ratio' is supported")
        if expected.k != int(k):
            raise ValueError(f"the expected table is for k={expected.k}, the map for k={k}")
        if value_max is None:
            value_max = 1024.0
    lo, hi, k, min_gap, chunk_rows = int(lo), int(hi), int(k), int(min_gap), int(chunk_rows)
    n = hi - lo
    width = _check_sweep_args(k, width, chunk_rows)
    if task_mode == "regress":
        if value_max is None:
            raise ValueError("task_mode 'regress' needs value_max: the largest value a candidate may contribute")
        vmax = float(value_max)
    else:
        vmax = 1.0 if expected is None else float(value_max)
    if not 0.0 < vmax <= float(1 << 20):
        raise ValueError("value_max must be in (0, 2^20]")
    mask = _plane_mask(planes)
    if (row_window is None) != (col_window is None):
        raise ValueError("row_window and col_window go together")
    if row_window is None:
        rows = cols = (lo, n)
    else:
        rows, cols = (int(row_window[0]), int(row_window[1])), (int(col_window[0]), int(col_window[1]))
        inside = all(w[1] >= 1 and lo <= w[0] and w[0] + w[1] <= hi for w in (rows, cols))
        if not inside or not (rows[0] + rows[1] <= cols[0] or cols[0] + cols[1] <= rows[0]):
            raise ValueError(f"row_window and col_window must be two disjoint (lo, n) windows inside [{lo}, {hi})")
    if n >= 1:
        _check_args(n, k, min_gap)
    m = n - (k - 1) * (min_gap - 1)
    if m >= k and math.comb(m, k - 2) * vmax >= float(1 << 31):
        raise ValueError(f"a cell may receive C({m}, {k - 2}) = {math.comb(m, k - 2)} candidates of value <= {vmax}: the sum's capacity of 2^31 "
                         "per cell is not enough (sweep a smaller region)")
    model.eval()
    dev = model.layer_norm1.weight.device
    total = kway_count(n, k, min_gap) if n >= 1 else 0
    if total == 0:
        out = _empty_map(max(rows[1], 0), max(cols[1], 0), mask, dev)
        out.update(n_candidates=0, n_excluded=0, n_rejected=0)
        return out
    chunk_rows = min(chunk_rows, total)
    pm = PairMap(rows, cols, mask, vmax=vmax, threshold=threshold, device=dev)
    tally = _tally(dev, "n_excluded")
    rows = lambda r0, count, buf, _: kway_rows(lo, n, k, min_gap, rank0=r0, count=count, width=width, out=buf)
    value = lambda r0, x: act(model(x).reshape(-1))                      # a map takes values, not logits
    if expected is not None:
        offset, scale = expected.table(mode, min_count, device=dev)
        value = lambda r0, x: expected.strata.enrich(x, act(model(x).reshape(-1)), offset, scale)
    with _pinned(model):
        for _, x, v, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev, flags=False), rows, exclude, tally, value):
            pm.update(x, v, skip)
    out = pm.result()
    out.pop("n_rows")
    out.update(n_candidates=total, **_counted(tally), n_rejected=int(out["n_rejected"].item()))
    return out


# ---- cluster completion: the bins that best extend clusters of 1 to 31 loci ------------------------------------------
MAX_CLUSTER = _lib.MAX_LONG_L - 1          # a cluster leaves room for one free node in a row of 32


def _check_complete_args(A: int, S: int, n: int, free: int, min_gap: int):
    if not (A >= 0 and 1 <= S <= MAX_CLUSTER and n >= 1 and 1 <= free <= _lib.MAX_L and min_gap >= 1):
        raise ValueError(f"need A >= 0, 1 <= S <= {MAX_CLUSTER}, n >= 1, 1 <= free <= {_lib.MAX_L}, min_gap >= 1 "
                         f"(A={A} S={S} n={n} free={free} min_gap={min_gap})")


def completion_count(A: int, S: int, n: int, free: int, min_gap: int) -> int:
    """Number of global ranks of a cluster table [A, S]: A * C_f with C_f = C(n - (free - 1)(min_gap - 1), free), the gap-constrained
    subsets of size ``free`` of a region of n nodes; a total >= 2^63 is refused (ValueError), not truncated."""
    A, S, n, free, min_gap = int(A), int(S), int(n), int(free), int(min_gap)
    _check_complete_args(A, S, n, free, min_gap)
    total = A * _free_count(n, free, min_gap)
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (A={A} n={n} free={free} min_gap={min_gap}) do not fit 63 bits")
    return total


def completion_unrank(rank: int, cluster, lo: int, n: int, free: int, min_gap: int) -> Tuple[Tuple[int, ...], bool]:
    """(row, valid) of one cluster's candidate of FREE rank ``rank`` (a global rank g is cluster g // C_f, free rank g % C_f), in
    Python integers (no GPU).  ``cluster``: its ids; as in the library only the run before the first zero counts (0 to 31 ids).  The row
    is those ids and the free part -- the gap-constrained subset of size ``free`` of [lo, lo + n) of that lexicographic rank -- sorted
    ascending, duplicates kept.  It is valid iff the cluster has an id, its ids are non-descending and every adjacent difference of
    the row is >= min_gap.  A cluster that descends somewhere is not merged: its ids in their order, then the free part, invalid."""
    ids = []
    for v in cluster:
        if int(v) == 0:
            break
        ids.append(int(v))
    lo, n, free, min_gap = int(lo), int(n), int(free), int(min_gap)
    _check_complete_args(1, max(len(ids), 1), n, free, min_gap)
    part = list(_subset_unrank(_checked_rank(rank, _free_count(n, free, min_gap)), lo, n, free, min_gap))
    ascending = all(a <= b for a, b in zip(ids, ids[1:]))
    row = tuple(sorted(ids + part)) if ascending else tuple(ids + part)
    return row, bool(ids) and ascending and all(b - a >= min_gap for a, b in zip(row, row[1:]))


def _cluster_table(clusters, device, limit: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """(int64 [A, S] on the device, max_a s_a): every row's non-zero ids sorted ascending, zeros last, S = max(1, max_a s_a).
    ``limit``: the most ids a cluster may hold, default MAX_CLUSTER (completion adds a node; decomposition, which adds none, passes 32).
    ``clusters``: a list of id lists (of any lengths), or an integer array / tensor zero-padded to a common width (1-D = single ids).
    Host inputs are measured on the host; a device tensor costs one small read-back (its longest row), before anything is launched
    by the library."""
    ragged = isinstance(clusters, (list, tuple)) and any(isinstance(c, (list, tuple)) or getattr(c, "ndim", 0) >= 1 for c in clusters)
    if isinstance(clusters, (list, tuple)) and len(clusters) == 0:
        t = torch.zeros(0, 1, dtype=torch.long)
    elif ragged:
        rows = [[int(v) for v in c] for c in clusters]
        width = max([len(r) for r in rows] + [1])
        t = torch.zeros(len(rows), width, dtype=torch.long)
        for a, r in enumerate(rows):
            t[a, :len(r)] = torch.tensor(r, dtype=torch.long)
    else:
        t = torch.as_tensor(clusters)
        if t.dim() == 1:
            t = t.view(-1, 1)
        if t.dim() != 2 or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("clusters must be a list of id lists or an integer [A, S] (or [A]) tensor or array")
        t = t.to(torch.long)
    if t.shape[1] == 0:
        t = torch.zeros(t.shape[0], 1, dtype=torch.long, device=t.device)
    s_max = int((t != 0).sum(dim=1).max()) if t.shape[0] else 0
    limit = MAX_CLUSTER if limit is None else int(limit)
    if s_max > limit:
        raise ValueError(f"a cluster has {s_max} ids: at most {limit} are supported")
    t = t.to(device)
    big = torch.iinfo(torch.long).max                                    # zeros behind every id, then back to zero
    t = torch.where(t == 0, torch.full_like(t, big), t).sort(dim=1).values[:, :max(s_max, 1)]
    return torch.where(t == big, torch.zeros_like(t), t).contiguous(), s_max


def _complete_rows(table: torch.Tensor, lo: int, n: int, free: int, min_gap: int, rank0: int, count: Optional[int], ranks, width: int,
                   out, flag_out) -> Tuple[torch.Tensor, torch.Tensor]:
    """matcha_kway_complete_rows on a table that is already in the library's form."""
    lib = _lib.load()
    A, S = int(table.shape[0]), int(table.shape[1])
    total = completion_count(A, S, n, free, min_gap)
    if not S + free <= width <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [{S + free}, {_lib.MAX_LONG_L}] (the longest cluster and the free part; got {width})")
    count = _rank_range(total, rank0, count, ranks)
    device = table.device
    x, flag = _row_buffers(count, width, device, out, flag_out, "completion_rows")
    if not x.is_cuda:
        raise _lib.MatchaHipError("completion_rows needs a cuda device (no CPU fallback)")
    with torch.cuda.device(device):
        _lib.check(lib.matcha_kway_complete_rows(_lib.ptr(table), A, S, int(lo), n, free, min_gap, int(rank0), _lib.ptr(ranks), count, width,
                                                 _lib.ptr(x), _lib.ptr(flag), _stream(device)), "matcha_kway_complete_rows")
    return x, flag


def completion_rows(clusters, lo: int, n: int, free: int, min_gap: int, rank0: int = 0, count: Optional[int] = None,
                    ranks: Optional[torch.Tensor] = None, width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None,
                    flag_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x int64 [count, width], flag int32 [count]) on the device: the candidates of the global ranks rank0 .. rank0 + count - 1, or
    of the device list ``ranks`` (a rank outside [0, A * C_f) gives an all-zero row with its flag set); flag != 0 marks an invalid
    candidate.  ``clusters``: a list of id lists of 0 to 31 ids each, or an integer [A, S] array / tensor zero-padded (each row is
    sorted here, zeros last).  ``width``: from (longest cluster + free), the default, up to 32.  ``out`` / ``flag_out`` reuse buffers
    of at least count * width / count elements."""
    if isinstance(clusters, torch.Tensor) and clusters.is_cuda and ranks is None and out is None:
        device = clusters.device
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        device = ranks.device
    elif out is not None:
        device = out.device
    n, free, min_gap = int(n), int(free), int(min_gap)
    _check_complete_args(0, 1, n, free, min_gap)
    table, s_max = _cluster_table(clusters, device)
    width = int(max(s_max, 1) + free if width is None else width)
    return _complete_rows(table, lo, n, free, min_gap, rank0, count, ranks, width, out, flag_out)


def completion_sweep(model, clusters, lo: int, hi: int, free: int = 1, min_gap: int = 1, top: int = 20, chunk_rows: Optional[int] = None,
                     width: Optional[int] = None, exclude=None, task_mode: str = "class") -> dict:
    """For every cluster (``clusters``: a list of id lists of 1 to 31 ids each, or a zero-padded integer [A, S] array / tensor) score
    all its completions by a gap-constrained subset of size ``free`` (1 .. 8) of the partner region [lo, hi) and keep the ``top`` best
    PER CLUSTER: which further bin, or set of bins, most plausibly belongs to it.  Clusters may lie inside the region, outside it or
    across chromosomes, and differ in size.

    All candidates are scored at ONE width (a logit depends on its batch's width: pads are attended): ``width``, default (longest
    cluster + free), at most 32.  Up to 8 it is model(x)'s forward for short rows, beyond it the long forward.

    Returns anchored_sweep's keys, on the model's device and best first within each cluster, with K = min(top, C_f): ``rows`` int64
    [A, K, width], ``logit`` and ``proba`` [A, K], ``rank`` int64 [A, K] (the FREE rank; decode with completion_unrank), ``count``
    int64 [A], and ``added`` int64 [A, K, free]: the free ids of each kept candidate.  Beyond count[a] the rank is -1 and everything
    else 0.  The integers ``n_candidates`` = A * C_f, ``n_invalid`` (a free node on or within the gap of a cluster id, a cluster that
    breaks the gap itself or has no id; scored, never kept) and ``n_excluded`` (valid candidates found in ``exclude``, a HyperedgeSet).

    ``chunk_rows``: None = 2^20 rows up to width 8 and min(2^20, 2^21 // width) beyond (about 3.1 KB of workspace per token); an
    explicit value the long forward cannot take is a ValueError before anything is launched.  The result does not depend on it.
    Eval mode and the loop (see the module's docstring) with the completion rows and SegTopK.update: nothing synchronises until the
    end, where the node-id check of the whole sweep is raised once (IndexError, also for a cluster id beyond the model's tables)."""
    act = _activation(task_mode)
    lo, hi, free, min_gap, top = int(lo), int(hi), int(free), int(min_gap), int(top)
    n = hi - lo
    if not 1 <= free <= _lib.MAX_L or min_gap < 1:
        raise ValueError(f"need 1 <= free <= {_lib.MAX_L} and min_gap >= 1 (free={free} min_gap={min_gap})")
    if width is not None and not free + 1 <= int(width) <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [longest cluster + free, {_lib.MAX_LONG_L}] (got {width})")
    if top < 1 or (chunk_rows is not None and int(chunk_rows) < 1):
        raise ValueError("top and chunk_rows must be >= 1")
    model.eval()
    dev = model.layer_norm1.weight.device
    table, s_max = _cluster_table(clusters, dev)
    A, S = int(table.shape[0]), int(table.shape[1])
    width = int(max(s_max, 1) + free if width is None else width)
    if not S + free <= width <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [{S + free}, {_lib.MAX_LONG_L}]: the longest cluster has {s_max} ids and free = {free} (got {width})")
    chunk_rows = _long_chunk_rows(model, chunk_rows, width)
    total = completion_count(A, S, n, free, min_gap) if n >= 1 else 0
    cf = total // A if A else 0
    K = min(top, cf)
    if total == 0:
        return {**_empty_segments(A, K, width, dev), "added": torch.zeros(A, K, free, dtype=torch.long, device=dev), "n_candidates": 0,
                "n_invalid": 0, "n_excluded": 0}
    chunk_rows = min(chunk_rows, total)
    sel = SegTopK(A, K, cf, chunk_rows, dev)
    tally = _tally(dev, "n_invalid", "n_excluded")
    rows = lambda g0, count, buf, fbuf: _complete_rows(table, lo, n, free, min_gap, g0, count, None, width, buf, fbuf)
    with _pinned(model):
        for g0, _, logits, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev), rows, exclude, tally):
            sel.update(logits, g0, skip)
    logit, grank, count = sel.read()
    rows, _ = _complete_rows(table, lo, n, free, min_gap, 0, None, grank.view(-1), width, None, None)
    # the added bins: the same ranks through the s_a = 0 form of the rows kernel (a table of empty clusters: the free part alone)
    added, _ = _complete_rows(torch.zeros(A, 1, dtype=torch.long, device=dev), lo, n, free, min_gap, 0, None, grank.view(-1), free + 1, None, None)
    rank, proba = _per_segment(grank, logit, cf, act)
    return {"rows": rows.view(A, K, width), "logit": logit, "proba": proba, "rank": rank, "count": count,
            "added": added.view(A, K, free + 1)[:, :, :free].contiguous(), "n_candidates": total, **_counted(tally)}


# ---- cluster decomposition: the sub-hyperedges of clusters of up to 32 loci ------------------------------------------
MAX_SUBSET_CLUSTER = _lib.MAX_LONG_L       # nothing is added to a cluster here, so it may fill a row of 32
_MODES = {"keep": 0, "drop": 1}


def _check_subset_args(A: int, S: int, m: int, complement: int):
    if not (A >= 0 and 2 <= S <= MAX_SUBSET_CLUSTER and complement in (0, 1) and (1 if complement else 2) <= m <= _lib.MAX_L):
        raise ValueError(f"need A >= 0, 2 <= S <= {MAX_SUBSET_CLUSTER}, complement 0 (keep, 2 <= m <= {_lib.MAX_L}) or 1 (drop, 1 <= m <= {_lib.MAX_L}) "
                         f"(A={A} S={S} m={m} complement={complement})")


def subset_count(A: int, S: int, m: int, complement: int = 0) -> int:
    """Number of global ranks of a cluster table [A, S]: A * C(S, m), the m-subsets of the S positions of every row; a total >= 2^63
    is refused (ValueError), not truncated."""
    A, S, m, complement = int(A), int(S), int(m), int(complement)
    _check_subset_args(A, S, m, complement)
    total = A * math.comb(S, m)
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (A={A} S={S} m={m}) do not fit 63 bits")
    return total


def _choice_unrank(rank: int, S: int, m: int) -> Tuple[int, ...]:
    """The m-subset of the positions [0, S) of lexicographic rank ``rank``."""
    return _subset_unrank(rank, 0, S, m, 1)


def subset_unrank(rank: int, cluster, m: int, complement: int = 0, min_gap: int = 1) -> Tuple[Tuple[int, ...], bool]:
    """(row, valid) of the candidate of CHOICE rank ``rank`` of one cluster row (a global rank g is cluster g // C(S, m), choice rank
    g % C(S, m)), in Python integers (no GPU).  ``cluster``: a row of the table, S = its length (at least 2): its ids are the run
    before the first zero.  The choice is the m-subset of the positions [0, S) of that lexicographic rank; the row is the ids at the
    chosen positions (complement 0, keep) or at all others (complement 1, drop), in position order.  It is valid iff every chosen
    position holds an id, the row has at least 2 ids, the cluster's ids are non-descending and every adjacent difference of the row
    is >= min_gap.  A choice that reaches past the ids gives the empty row, invalid."""
    cluster = [int(v) for v in cluster]
    S, m, complement, min_gap, rank = max(len(cluster), 2), int(m), int(complement), int(min_gap), int(rank)
    _check_subset_args(1, S, m, complement)
    if min_gap < 1:
        raise ValueError("min_gap must be >= 1")
    rank = _checked_rank(rank, math.comb(S, m))
    ids = []
    for v in cluster:
        if v == 0:
            break
        ids.append(v)
    pos = _choice_unrank(rank, S, m)
    if any(p >= len(ids) for p in pos):
        return (), False
    chosen = set(pos)
    row = tuple(ids[p] for p in range(len(ids)) if (p in chosen) != bool(complement))
    ascending = all(a <= b for a, b in zip(ids, ids[1:]))
    return row, len(row) >= 2 and ascending and all(b - a >= min_gap for a, b in zip(row, row[1:]))


def _subset_table(clusters, device) -> Tuple[torch.Tensor, int]:
    """_cluster_table for clusters of up to 32 ids, at least 2 columns wide."""
    t, s_max = _cluster_table(clusters, device, limit=MAX_SUBSET_CLUSTER)
    if t.shape[1] < 2:
        t = torch.cat([t, torch.zeros(t.shape[0], 2 - t.shape[1], dtype=torch.long, device=t.device)], dim=1).contiguous()
    return t, s_max


def _subset_rows(table: torch.Tensor, m: int, complement: int, min_gap: int, rank0: int, count: Optional[int], ranks, width: int, out,
                 flag_out) -> Tuple[torch.Tensor, torch.Tensor]:
    """matcha_cluster_subset_rows on a table that is already in the library's form."""
    lib = _lib.load()
    A, S = int(table.shape[0]), int(table.shape[1])
    total = subset_count(A, S, m, complement)
    if min_gap < 1:
        raise ValueError("min_gap must be >= 1")
    least = max(S - m, 1) if complement else m
    if not least <= width <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [{least}, {_lib.MAX_LONG_L}] (keep: m, drop: S - m; got {width})")
    count = _rank_range(total, rank0, count, ranks)
    device = table.device
    x, flag = _row_buffers(count, width, device, out, flag_out, "subset_rows")
    if not x.is_cuda:
        raise _lib.MatchaHipError("subset_rows needs a cuda device (no CPU fallback)")
    with torch.cuda.device(device):
        _lib.check(lib.matcha_cluster_subset_rows(_lib.ptr(table), A, S, m, complement, min_gap, int(rank0), _lib.ptr(ranks), count, width,
                                                  _lib.ptr(x), _lib.ptr(flag), _stream(device)), "matcha_cluster_subset_rows")
    return x, flag


def subset_rows(clusters, m: int, complement: int = 0, min_gap: int = 1, rank0: int = 0, count: Optional[int] = None,
                ranks: Optional[torch.Tensor] = None, width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None,
                flag_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x int64 [count, width], flag int32 [count]) on the device: the candidates of the global ranks rank0 .. rank0 + count - 1, or
    of the device list ``ranks`` (a rank outside [0, A * C(S, m)) gives an all-zero row with its flag set); flag != 0 marks an
    invalid candidate.  ``clusters``: a list of id lists of 0 to 32 ids each, or an integer [A, S] array / tensor zero-padded (each
    row is sorted here, zeros last); S = the longest cluster, at least 2.  ``width``: keep, from m (the default) to 32; drop, from
    S - m to 32, default S.  ``out`` / ``flag_out`` reuse buffers of at least count * width / count elements."""
    if isinstance(clusters, torch.Tensor) and clusters.is_cuda and ranks is None and out is None:
        device = clusters.device
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        device = ranks.device
    elif out is not None:
        device = out.device
    m, complement, min_gap = int(m), int(complement), int(min_gap)
    _check_subset_args(0, 2, m, complement)
    table, _ = _subset_table(clusters, device)
    width = int((table.shape[1] if complement else m) if width is None else width)
    return _subset_rows(table, m, complement, min_gap, rank0, count, ranks, width, out, flag_out)


class SubsetSupport:
    """Per-locus support on the device (csrc/sweep.hip's subset_support_update_kernel): for the ``A`` clusters of a table [A, S] and
    choices of ``m`` positions, two int64 planes [A, S] -- over the accepted rows whose choice contains the position, the sum of their
    values in PairMap's fixed point (32 fractional bits) and their number.  Integer atomics only: bit for bit the same whatever the
    order of the updates and however the ranks were cut into them.  ``vmax``: the largest value accepted, 0 < vmax <= 2^20."""

    def __init__(self, A: int, S: int, m: int, vmax: float = 1.0, device="cuda"):
        lib = _lib.load()
        self.A, self.S, self.m, self.vmax = int(A), int(S), int(m), float(vmax)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("SubsetSupport needs a cuda device (no CPU fallback)")
        fits = 1 <= self.A <= 1 << 40 and abs(self.S) < 1 << 31 and abs(self.m) < 1 << 31
        self._dims = (self.A, self.S, self.m, self.vmax)
        self.bytes = int(lib.matcha_subset_support_bytes(*self._dims)) if fits else 0
        if self.bytes == 0:
            raise ValueError(f"SubsetSupport: need 1 <= A <= 2^40, 2 <= S <= {MAX_SUBSET_CLUSTER}, 1 <= m <= {_lib.MAX_L} and 0 < vmax <= 2^20 "
                             f"(A={A} S={S} m={m} vmax={vmax})")
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_support_init(_lib.ptr(self.state), self.bytes, *self._dims, _stream(self.device)), "matcha_subset_support_init")

    def update(self, value: torch.Tensor, g0: int, skip: Optional[torch.Tensor] = None):
        """``value`` float32 [n] on the device, row i of global rank g0 + i (cluster (g0 + i) // C(S, m), the choice of the remainder);
        ``skip`` int32 / bool [n], non-zero = the row contributes nothing.  A row whose value is NaN, negative or > vmax is counted as
        rejected.  Enqueued on the current stream; nothing is read back."""
        lib = _lib.load()
        value, skip = _scores_and_skip(value, skip, self.state.device, "SubsetSupport")
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_support_update(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(value), _lib.ptr(skip),
                                                        value.numel(), int(g0), _stream(self.device)), "matcha_subset_support_update")

    def read(self) -> dict:
        """'sum' int64 [A, S] (fixed point, value * 2^32), 'count' int64 [A, S] and 'counters' int64 [2] = (accepted rows, rejected
        rows), on the device and without a synchronisation."""
        lib = _lib.load()
        total = torch.empty(self.A, self.S, dtype=torch.long, device=self.device)
        count = torch.empty(self.A, self.S, dtype=torch.long, device=self.device)
        counters = torch.empty(2, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_support_read(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(total), _lib.ptr(count),
                                                      _lib.ptr(counters), _stream(self.device)), "matcha_subset_support_read")
        return {"sum": total, "count": count, "counters": counters}


class SubsetPairSupport:
    """Per-pair support on the device (csrc/sweep.hip's subset_pair_update_kernel), SubsetSupport's twin: for the ``A``
    clusters of a table [A, S] and choices of ``m`` positions, 2 <= m <= 8, two int64 planes [A, P], P = S (S - 1) / 2 -- per pair of
    positions i < j, over the accepted rows whose choice contains both, the sum of their values in the same fixed point and their
    number.  Only the upper triangle is kept, row-major: pair (i, j) is column i (2 S - i - 1) / 2 + (j - i - 1), the order of
    ``pair_index``.  Integer atomics only: bit for bit the same whatever the order of the updates and however the ranks were cut."""

    def __init__(self, A: int, S: int, m: int, vmax: float = 1.0, device="cuda"):
        lib = _lib.load()
        self.A, self.S, self.m, self.vmax = int(A), int(S), int(m), float(vmax)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("SubsetPairSupport needs a cuda device (no CPU fallback)")
        fits = 1 <= self.A <= 1 << 40 and abs(self.S) < 1 << 31 and abs(self.m) < 1 << 31
        self._dims = (self.A, self.S, self.m, self.vmax)
        self.bytes = int(lib.matcha_subset_pair_bytes(*self._dims)) if fits else 0
        if self.bytes == 0:
            raise ValueError(f"SubsetPairSupport: need 1 <= A <= 2^40, 2 <= S <= {MAX_SUBSET_CLUSTER}, 2 <= m <= {_lib.MAX_L} and 0 < vmax <= 2^20 "
                             f"(A={A} S={S} m={m} vmax={vmax})")
        self.P = self.S * (self.S - 1) // 2
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_pair_init(_lib.ptr(self.state), self.bytes, *self._dims, _stream(self.device)), "matcha_subset_pair_init")

    @staticmethod
    def pair_index(S: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(i, j) int64 [P] each: the positions of the packed columns, torch.triu_indices(S, S, 1) in row-major order."""
        S = int(S)
        i, j = torch.triu_indices(S, S, 1)
        assert torch.equal(i * (2 * S - i - 1) // 2 + (j - i - 1), torch.arange(S * (S - 1) // 2))     # the kernel's cell formula
        return i.to(device), j.to(device)

    def update(self, value: torch.Tensor, g0: int, skip: Optional[torch.Tensor] = None):
        """SubsetSupport.update's contract: ``value`` float32 [n] on the device, row i of global rank g0 + i; ``skip`` int32 / bool [n],
        non-zero = the row contributes nothing; a row whose value is NaN, negative or > vmax is counted as rejected.  Enqueued on the
        current stream; nothing is read back."""
        lib = _lib.load()
        value, skip = _scores_and_skip(value, skip, self.state.device, "SubsetPairSupport")
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_pair_update(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(value), _lib.ptr(skip),
                                                     value.numel(), int(g0), _stream(self.device)), "matcha_subset_pair_update")

    def read(self) -> dict:
        """'sum' int64 [A, P] (fixed point, value * 2^32), 'count' int64 [A, P] and 'counters' int64 [2] = (accepted rows, rejected
        rows), on the device and without a synchronisation."""
        lib = _lib.load()
        total = torch.empty(self.A, self.P, dtype=torch.long, device=self.device)
        count = torch.empty(self.A, self.P, dtype=torch.long, device=self.device)
        counters = torch.empty(2, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_subset_pair_read(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(total), _lib.ptr(count),
                                                   _lib.ptr(counters), _stream(self.device)), "matcha_subset_pair_read")
        return {"sum": total, "count": count, "counters": counters}


@functools.lru_cache(maxsize=None)
def _pair_square_map(S: int) -> torch.Tensor:
    """int64 [S * S] on the host: for every cell of the row-major S x S square the column of the packed upper triangle that holds its
    pair, P = S (S - 1) / 2 (a zero column appended to the plane) on the diagonal."""
    pi, pj = SubsetPairSupport.pair_index(S)
    square = torch.full((S, S), S * (S - 1) // 2, dtype=torch.long)
    square[pi, pj] = square[pj, pi] = torch.arange(pi.numel())
    return square.view(-1)


def decomposition_sweep(model, clusters, m: int, mode: str = "keep", min_gap: int = 1, top: int = 20, chunk_rows: Optional[int] = None,
                        width: Optional[int] = None, exclude=None, task_mode: str = "class", support: bool = True,
                        pair_support: bool = False) -> dict:
    """For every cluster (``clusters``: a list of id lists of up to 32 ids each, or a zero-padded integer [A, S] array / tensor) score
    all candidates made of its OWN ids and keep the ``top`` best PER CLUSTER.  mode 'keep': the sub-hyperedges of ``m`` of its ids
    (2 <= m <= 8) -- which triples or quadruples inside the cluster are real simultaneous contacts.  mode 'drop': the cluster with
    ``m`` of its ids taken out (1 <= m <= 8) -- which locus does not belong -- scored beside the whole cluster.

    The clusters are grouped by size and every size s is swept by itself (a table [A_s, s], C(s, m) candidates per cluster), so a
    ragged file wastes no rank and no all-zero row is scored; results come back in the input order.  A cluster too small (keep:
    s < m; drop: s - m < 2) never reaches the device and has count 0.  All groups are scored at ONE width (a logit depends on its
    batch's width): keep, ``width`` from m (the default) to 8; drop, from the longest cluster (the default, at least 2) to 32.  Up
    to 8 it is model(x)'s forward for short rows with the large-batch route pinned, beyond it the long forward.

    Returns, on the model's device and best first within each cluster, with K = min(top, the largest C(s_a, m) swept): ``rows`` int64
    [A, K, width], ``logit`` and ``proba`` [A, K], ``rank`` int64 [A, K] (the rank within C(s_a, m); decode with subset_unrank on the
    cluster's s_a ids), ``count`` int64 [A] and ``chosen`` int64 [A, K, m]: the kept (keep) or dropped (drop) ids.  Beyond count[a]
    the rank is -1 and everything else 0.  With ``support`` (task_mode 'class' only: the planes take the sigmoid's output):
    ``support_sum`` float64 and ``support_count`` int64 [A, S_max] -- per locus of the cluster, the summed probability and the number
    of the valid, non-excluded candidates whose choice contains it -- and ``support_mean`` float32, their quotient (0 where the count
    is 0): in keep mode how credible the sub-hyperedges through the locus are, in drop mode how credible the cluster is without it.
    With ``pair_support`` (task_mode 'class' and m >= 2 only): ``pair_sum`` float64 and ``pair_count`` int64
    [A, S_max, S_max] -- per PAIR of loci (i, j) of the cluster, the summed probability and the number of the valid, non-excluded
    candidates whose choice contains both -- and ``pair_mean`` float32, their quotient (0 where the count is 0).  In keep mode cell
    (i, j) is the mean probability of the sub-hyperedges of m loci that contain both locus i and locus j; in drop mode the mean
    probability of the cluster with both (and m - 2 others) taken out.  All three are symmetric with a zero diagonal, zero at
    positions >= s_a and in a cluster not swept; cell for cell the layout of the attention map of the same cluster.  They are dense:
    together 20 * A * S_max^2 bytes.
    In drop mode ``full_logit`` and ``full_proba`` [A]: the whole cluster at the same width (0 for a cluster not swept).  The
    integers ``n_candidates``, ``n_invalid`` (candidates that break the gap rule; scored, never kept) and ``n_excluded`` (valid
    candidates found in ``exclude``, a HyperedgeSet).

    ``chunk_rows`` as in completion_sweep; the result does not depend on it, bit for bit.  Eval mode and the loop (see the module's
    docstring), once per size with buffers sized for the largest, into SegTopK and the support planes: nothing synchronises until
    the end, where the node-id check of the whole sweep is raised once."""
    act = _activation(task_mode)
    if mode not in _MODES:
        raise ValueError("mode must be 'keep' or 'drop'")
    if support and task_mode == "regress":
        raise ValueError("the support planes take the sigmoid's output: task_mode 'regress' needs support=False")
    complement = _MODES[mode]
    m, min_gap, top = int(m), int(min_gap), int(top)
    if pair_support and (task_mode != "class" or m < 2):
        raise ValueError("the pair planes take the sigmoid's output and a choice of at least two positions: pair_support needs "
                         f"task_mode 'class' and m >= 2 (task_mode='{task_mode}' m={m})")
    if not (1 if complement else 2) <= m <= _lib.MAX_L or min_gap < 1:
        raise ValueError(f"need {1 if complement else 2} <= m <= {_lib.MAX_L} in mode '{mode}' and min_gap >= 1 (m={m} min_gap={min_gap})")
    if top < 1 or (chunk_rows is not None and int(chunk_rows) < 1):
        raise ValueError("top and chunk_rows must be >= 1")
    model.eval()
    dev = model.layer_norm1.weight.device
    table, s_max = _subset_table(clusters, dev)
    A, S_max = int(table.shape[0]), int(table.shape[1])
    least, most = (max(s_max, 2), _lib.MAX_LONG_L) if complement else (m, _lib.MAX_L)
    width = int(least if width is None else width)
    if not least <= width <= most:
        raise ValueError(f"width must be in [{least}, {most}] in mode '{mode}' (m = {m}, the longest cluster has {s_max} ids; got {width})")
    chunk_rows = _long_chunk_rows(model, chunk_rows, width)
    sizes = (table != 0).sum(dim=1).cpu() if A else torch.zeros(0, dtype=torch.long)      # one small read-back, before anything is launched
    groups = []
    for s in sorted(set(sizes.tolist())):
        if (s - m >= 2) if complement else (s >= m):
            idx = torch.nonzero(sizes == s).view(-1).to(dev)
            groups.append((s, idx, math.comb(s, m)))
    pair_map = {}                                                        # per size: square cell -> packed column; one copy, before anything is launched
    if pair_support and groups:
        maps = [_pair_square_map(s) for s, _, _ in groups]
        pair_map = dict(zip([s for s, _, _ in groups], torch.cat(maps).to(dev).split([int(t.numel()) for t in maps])))
    K = min(top, max([cm for _, _, cm in groups] + [0]))
    out = {**_empty_segments(A, K, width, dev), "chosen": torch.zeros(A, K, m, dtype=torch.long, device=dev)}
    if support:
        out["support_sum"] = torch.zeros(A, S_max, dtype=torch.float64, device=dev)
        out["support_count"] = torch.zeros(A, S_max, dtype=torch.long, device=dev)
    if pair_support:
        out["pair_sum"] = torch.zeros(A, S_max, S_max, dtype=torch.long, device=dev)        # fixed point until the end
        out["pair_count"] = torch.zeros(A, S_max, S_max, dtype=torch.long, device=dev)
    if complement:
        out["full_logit"] = torch.zeros(A, dtype=torch.float32, device=dev)
    n_cand = sum(int(idx.numel()) * cm for _, idx, cm in groups)
    if groups:
        buffers = _buffers(min(chunk_rows, max(int(idx.numel()) * cm for _, idx, cm in groups)), width, dev)
    tally = _tally(dev, "n_invalid", "n_excluded")
    done = []
    with _pinned(model):
        for s, idx, cm in groups:
            tab = table[idx, :s].contiguous()
            A_s = int(tab.shape[0])
            total = A_s * cm
            sel = SegTopK(A_s, min(top, cm), cm, min(chunk_rows, total), dev)
            sup = SubsetSupport(A_s, s, m, 1.0, dev) if support else None
            psup = SubsetPairSupport(A_s, s, m, 1.0, dev) if pair_support else None
            rows = lambda g0, count, buf, fbuf: _subset_rows(tab, m, complement, min_gap, g0, count, None, width, buf, fbuf)
            for g0, _, logits, skip, _ in _chunks(model, total, chunk_rows, buffers, rows, exclude, tally):
                sel.update(logits, g0, skip)
                if sup is not None or psup is not None:
                    proba = torch.sigmoid(logits)
                    if sup is not None:
                        sup.update(proba, g0, skip)
                    if psup is not None:
                        psup.update(proba, g0, skip)
            done.append((s, idx, cm, tab, sel, sup, psup))
        if complement and groups:                                        # the whole clusters, all sizes in one batch: the sweep's width and route
            swept = torch.cat([idx for _, idx, _ in groups])
            whole = torch.zeros(int(swept.numel()), width, dtype=torch.long, device=dev)
            whole[:, :S_max] = table[swept]                              # width >= S_max in drop mode
            for a0 in range(0, int(swept.numel()), chunk_rows):
                out["full_logit"][swept[a0:a0 + chunk_rows]] = model(whole[a0:a0 + chunk_rows]).reshape(-1)
    for s, idx, cm, tab, sel, sup, psup in done:
        A_s, Ks = int(tab.shape[0]), min(top, cm)
        logit, grank, count = sel.read()
        rows, _ = _subset_rows(tab, m, complement, min_gap, 0, None, grank.view(-1), width, None, None)
        rank, proba = _per_segment(grank, logit, cm, act)
        if m == 1:                                                       # a choice of one position is its rank
            chosen = torch.where(rank >= 0, tab.gather(1, rank.clamp(min=0)), torch.zeros_like(rank)).view(A_s, Ks, 1)
        else:                                                            # the same ranks through the keep form of the rows kernel
            chosen = _subset_rows(tab, m, 0, 1, 0, None, grank.view(-1), m, None, None)[0].view(A_s, Ks, m)
        out["rows"][idx, :Ks] = rows.view(A_s, Ks, width)
        out["logit"][idx, :Ks] = logit
        out["proba"][idx, :Ks] = proba
        out["rank"][idx, :Ks] = rank
        out["count"][idx] = count
        out["chosen"][idx, :Ks] = chosen
        if sup is not None:
            planes = sup.read()
            out["support_sum"][idx, :s] = planes["sum"].to(torch.float64) / 4294967296.0
            out["support_count"][idx, :s] = planes["count"]
        if psup is not None:                                             # the packed upper triangles into both halves of the squares
            planes = psup.read()
            for key, packed in (("pair_sum", planes["sum"]), ("pair_count", planes["count"])):
                square = torch.nn.functional.pad(packed, (0, 1)).index_select(1, pair_map[s])
                out[key][idx, :s, :s] = square.view(A_s, s, s)
    if pair_support:
        out["pair_sum"] = out["pair_sum"].to(torch.float64) / 4294967296.0
        hit = out["pair_count"] > 0
        out["pair_mean"] = torch.where(hit, out["pair_sum"] / out["pair_count"].clamp(min=1).to(torch.float64),
                                       torch.zeros_like(out["pair_sum"])).to(torch.float32)
    if support:
        hit = out["support_count"] > 0
        out["support_mean"] = torch.where(hit, out["support_sum"] / out["support_count"].clamp(min=1).to(torch.float64),
                                          torch.zeros_like(out["support_sum"])).to(torch.float32)
    if complement:
        swept = torch.zeros(A, dtype=torch.bool, device=dev)
        for _, idx, _, _, _, _, _ in done:
            swept[idx] = True
        out["full_proba"] = torch.where(swept, act(out["full_logit"]), torch.zeros_like(out["full_logit"]))
    out.update(n_candidates=n_cand, **_counted(tally))
    return out


# ---- cluster growth: beam-search hubs of up to 32 loci from seed clusters ------------------------------------------------
MAX_BEAM = 64                              # slots per seed: one lane per column of a twin row (csrc/grow.hip)


def _check_grow_args(B: int, S: int):
    if not (1 <= B <= MAX_BEAM and 1 <= S <= MAX_CLUSTER):
        raise ValueError(f"need 1 <= B <= {MAX_BEAM} slots per seed and 1 <= S <= {MAX_CLUSTER} ids per slot (B={B} S={S})")


def grow_twins(beam: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [A * B, B] on the device, matcha_grow_twins on a beam table int64 [A, B, S] as it stands (nothing is sorted here): column
    j' < j of row a * B + j holds the one id of slot_j' \\ slot_j when the two slots of seed a are strictly ascending, non-empty and of
    one size, -1 when they are identical, 0 for no relation; columns j' >= j are 0.  ``out`` reuses a buffer of at least A * B * B
    elements."""
    lib = _lib.load()
    if beam.dim() != 3 or beam.dtype != torch.long:
        raise ValueError("beam must be an int64 [A, B, S] tensor")
    A, B, S = (int(v) for v in beam.shape)
    _check_grow_args(B, S)
    if not beam.is_cuda:
        raise _lib.MatchaHipError("grow_twins needs a cuda device (no CPU fallback)")
    beam = beam.contiguous()
    twin, _ = _row_buffers(A * B, B, beam.device, out, None, "grow_twins", flags=False)
    with torch.cuda.device(beam.device):
        _lib.check(lib.matcha_grow_twins(_lib.ptr(beam), A, B, S, _lib.ptr(twin), _stream(beam.device)), "matcha_grow_twins")
    return twin


def grow_twin_flags(twin: torch.Tensor, lo: int, n: int, flag: torch.Tensor, rank0: int = 0, count: Optional[int] = None) -> torch.Tensor:
    """ORs 2 into flag[i] (int32, as the rows kernel of cluster completion wrote it) when the candidate of global rank rank0 + i --
    entry g // n, free id lo + g % n -- is a twin by ``twin`` (grow_twins' table, int64 [A * B, B]).  ``count``: default everything
    from rank0; ``flag`` may be longer than count, what lies behind is untouched.  Returns flag."""
    lib = _lib.load()
    if twin.dim() != 2 or twin.dtype != torch.long or not twin.is_contiguous():
        raise ValueError("twin must be a contiguous int64 [A * B, B] tensor")
    B = int(twin.shape[1])
    _check_grow_args(B, 1)
    if int(twin.shape[0]) % B:
        raise ValueError("twin must have A * B rows of B columns")
    A, lo, n, rank0 = int(twin.shape[0]) // B, int(lo), int(n), int(rank0)
    if n < 1:
        raise ValueError(f"need n >= 1 (n={n})")
    total = A * B * n
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (A={A} B={B} n={n}) do not fit 63 bits")
    count = _rank_range(total, rank0, count, None)
    if flag.dtype != torch.int32 or not flag.is_contiguous() or flag.numel() < count or flag.device != twin.device:
        raise ValueError("flag must be a contiguous int32 tensor of at least count elements on twin's device")
    if not twin.is_cuda:
        raise _lib.MatchaHipError("grow_twin_flags needs a cuda device (no CPU fallback)")
    with torch.cuda.device(twin.device):
        _lib.check(lib.matcha_grow_twin_flags(_lib.ptr(twin), A, B, lo, n, rank0, count, _lib.ptr(flag), _stream(twin.device)),
                   "matcha_grow_twin_flags")
    return flag


def _grow_step(model, beam: torch.Tensor, lo: int, n: int, K: int, min_gap: int, width: int, exclude, chunk_rows: int, act,
               counters: torch.Tensor) -> dict:
    """One step on a beam int64 [A, B, S] on the model's device, A >= 1 and n >= 1: twin table, the loop over the completion rows with
    the twins flagged, one SegTopK per seed, the advance.  Nothing is read back; ``counters`` (device int64 [3]: invalid, twins,
    excluded) is added to.  The caller holds eval mode and ``_pinned``."""
    A, B, S = (int(v) for v in beam.shape)
    dev = beam.device
    table = beam.view(A * B, S)
    total = A * B * n
    chunk_rows = min(chunk_rows, total)
    twin = grow_twins(beam)
    sel = SegTopK(A, K, B * n, chunk_rows, dev)

    def rows(g0, count, buf, fbuf):
        x, flag = _complete_rows(table, lo, n, 1, min_gap, g0, count, None, width, buf, fbuf)
        return x, grow_twin_flags(twin, lo, n, flag, g0, count)

    tally = {"n_excluded": counters[2]}                                  # invalid rows and twins are told apart here, from the flag
    for g0, _, logits, skip, flag in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev), rows, exclude, tally):
        counters[0] += ((flag & 1) != 0).sum()
        counters[1] += (flag == 2).sum()                                 # valid candidates that are twins
        sel.update(logits, g0, skip)
    logit, grank, count = sel.read()
    rows, _ = _complete_rows(table, lo, n, 1, min_gap, 0, None, grank.view(-1), width, None, None)      # rank -1: an all-zero row
    rows = rows.view(A, K, width)
    rank, proba = _per_segment(grank, logit, B * n, act)
    kept, zero = rank >= 0, torch.zeros_like(rank)
    return {"rows": rows, "logit": logit, "proba": proba, "rank": rank,
            "parent": torch.where(kept, torch.div(rank, n, rounding_mode="floor"), zero), "added": torch.where(kept, lo + rank % n, zero),
            "count": count, "beam": rows[:, :, :S + 1].contiguous()}


def _empty_step(A: int, K: int, S: int, width: int, dev) -> dict:
    z = torch.zeros(A, K, dtype=torch.long, device=dev)
    return {**_empty_segments(A, K, width, dev), "parent": z, "added": z.clone(), "beam": torch.zeros(A, K, S + 1, dtype=torch.long, device=dev)}


def grow_step(model, beam, lo: int, hi: int, beam_out: Optional[int] = None, min_gap: int = 1, width: Optional[int] = None, exclude=None,
              chunk_rows: Optional[int] = None, task_mode: str = "class") -> dict:
    """One step of cluster growth.  ``beam`` int64 [A, B, S]: A seeds, B slots (1 .. 64) per seed, every slot a cluster of up to S ids
    (1 .. 31) ascending with zeros behind them, an all-zero slot empty; it is used as it stands.  Every slot is extended by every bin
    of [lo, hi) (cluster completion with free = 1; the candidate of slot j and bin lo + r has the seed's rank j n + r), candidates that
    a LOWER slot of the seed reaches too are flagged as twins, and per seed the K = min(beam_out, B n) best candidates that are valid,
    not twins and not in ``exclude`` are kept (``beam_out``: default B).

    All candidates are scored at ONE width, default S + 1, at most 32: up to 8 model(x)'s forward for short rows with the large-batch
    route pinned, beyond it the long forward.  Returns, on the model's device and best first within a seed, ``rows`` int64
    [A, K, width], ``logit``, ``proba``, ``rank`` (within the seed), ``parent`` (the slot extended) and ``added`` (the bin) [A, K],
    ``count`` int64 [A] and ``beam`` int64 [A, K, S + 1], the table of the next step; beyond count[a] the rank is -1 and everything
    else 0.  The integers ``n_candidates`` = A B n, ``n_invalid`` (completion_sweep's), ``n_twins`` (valid candidates flagged as
    twins) and ``n_excluded``.  ``chunk_rows`` as in completion_sweep, and the loop of the module's docstring; the result does not depend
    on the cut."""
    act = _activation(task_mode)
    lo, hi, min_gap = int(lo), int(hi), int(min_gap)
    n = hi - lo
    beam = torch.as_tensor(beam)
    if beam.dim() != 3 or beam.is_floating_point() or beam.dtype == torch.bool:
        raise ValueError("beam must be an integer [A, B, S] tensor or array")
    A, B, S = (int(v) for v in beam.shape)
    _check_grow_args(B, S)
    beam_out = B if beam_out is None else int(beam_out)
    if not 1 <= beam_out <= MAX_BEAM or min_gap < 1:
        raise ValueError(f"need 1 <= beam_out <= {MAX_BEAM} and min_gap >= 1 (beam_out={beam_out} min_gap={min_gap})")
    width = int(S + 1 if width is None else width)
    if not S + 1 <= width <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [{S + 1}, {_lib.MAX_LONG_L}]: a slot holds up to {S} ids and a bin is added (got {width})")
    chunk_rows = _long_chunk_rows(model, chunk_rows, width)
    model.eval()
    dev = model.layer_norm1.weight.device
    K = min(beam_out, B * max(n, 0))
    if A == 0 or n < 1:
        out = _empty_step(A, K, S, width, dev)
        out.update(n_candidates=0, n_invalid=0, n_twins=0, n_excluded=0)
        return out
    beam = beam.to(device=dev, dtype=torch.long).contiguous()
    counters = torch.zeros(3, dtype=torch.long, device=dev)
    with _pinned(model):
        out = _grow_step(model, beam, lo, n, K, min_gap, width, exclude, chunk_rows, act, counters)
    c = counters.tolist()
    out.update(n_candidates=A * B * n, n_invalid=c[0], n_twins=c[1], n_excluded=c[2])
    return out


def growth_sweep(model, seeds, lo: int, hi: int, max_size: int, beam: int = 8, min_gap: int = 1, width: Optional[int] = None, exclude=None,
                 chunk_rows: Optional[int] = None, task_mode: str = "class") -> dict:
    """Beam-search the most plausible hubs of up to ``max_size`` loci (2 .. 32) that contain a seed: every seed (``seeds`` in
    completion_sweep's ``clusters`` form, 1 to 31 ids each, of any sizes) is grown by one bin of [lo, hi) per step, ``beam`` (1 .. 64)
    hubs kept per seed and size (grow_step).  Step t runs on the seeds with s_a + t < max_size, the first with one slot per seed.

    Every step is scored at ONE width, default ``max_size``, at most 32 (a logit depends on its batch's width).  With T = max_size -
    (the fewest ids of a seed that has any) and B = beam it returns, on the model's device, level t of seed a holding its hubs of
    s_a + t + 1 loci best first: ``rows`` int64 [A, T, B, width], ``logit``, ``proba``, ``parent`` (the slot of level t - 1 a hub
    extends), ``added`` (the bin it adds) [A, T, B]; ``count`` and ``size`` int64 [A, T] (size = s_a + t + 1 where the level exists,
    else 0); ``path`` int64 [A, B, T]: for each hub of a seed's LAST level the bins added, in the order of addition, zeros behind;
    the integers ``n_candidates``, ``n_invalid``, ``n_twins``, ``n_excluded`` (summed over the steps) and ``steps``.  A seed with
    s_a >= max_size, or without an id, has no levels.  Slots beyond count are 0.

    Seed sizes are read on the host (a device tensor costs one small read-back before anything is launched); the counters stay on the
    device, nothing synchronises between steps, and the node-id check of the whole growth is raised once at the end (IndexError):
    ``_pinned`` is held across all steps."""
    act = _activation(task_mode)
    lo, hi, max_size, B, min_gap = int(lo), int(hi), int(max_size), int(beam), int(min_gap)
    n = hi - lo
    if not 2 <= max_size <= _lib.MAX_LONG_L:
        raise ValueError(f"max_size must be in [2, {_lib.MAX_LONG_L}] (got {max_size})")
    if not 1 <= B <= MAX_BEAM or min_gap < 1:
        raise ValueError(f"need 1 <= beam <= {MAX_BEAM} and min_gap >= 1 (beam={B} min_gap={min_gap})")
    width = int(max_size if width is None else width)
    if not max_size <= width <= _lib.MAX_LONG_L:
        raise ValueError(f"width must be in [max_size, {_lib.MAX_LONG_L}] (got {width} for max_size = {max_size})")
    chunk_rows = _long_chunk_rows(model, chunk_rows, width)
    model.eval()
    dev = model.layer_norm1.weight.device
    if isinstance(seeds, torch.Tensor) and seeds.is_cuda:
        seeds = seeds.cpu()                                              # the one read-back: sizes are host knowledge from here on
    table, _ = _cluster_table(seeds, "cpu")
    sizes = (table != 0).sum(dim=1)
    A = int(table.shape[0])
    grows = (sizes >= 1) & (sizes < max_size)
    T = max_size - int(sizes[sizes >= 1].min()) if bool((sizes >= 1).any()) else 0
    T = max(T, 0)
    zf = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    zl = lambda *shape: torch.zeros(*shape, dtype=torch.long, device=dev)
    out = {"rows": zl(A, T, B, width), "logit": zf(A, T, B), "proba": zf(A, T, B), "parent": zl(A, T, B), "added": zl(A, T, B),
           "count": zl(A, T), "size": zl(A, T), "path": zl(A, B, T)}
    steps = torch.where(grows, max_size - sizes, torch.zeros_like(sizes))                # levels per seed, on the host
    n_cand, n_steps = 0, 0
    counters = torch.zeros(3, dtype=torch.long, device=dev)
    if n >= 1 and T > 0:
        t_idx = torch.arange(T).view(1, -1)
        out["size"] = torch.where(t_idx < steps.view(-1, 1), sizes.view(-1, 1) + t_idx + 1, torch.zeros(A, T, dtype=torch.long)).to(dev)
        with _pinned(model):
            active = torch.nonzero(steps > 0).view(-1)                   # host indices of the seeds of step 0
            cur = table[active].to(dev).view(-1, 1, int(table.shape[1]))
            for t in range(T):
                if t:
                    keep = torch.nonzero(steps[active] > t).view(-1)     # a seed that has reached max_size leaves
                    if keep.numel() == 0:
                        break
                    if keep.numel() < active.numel():
                        cur = cur[keep.to(dev)]
                        active = active[keep]
                S_t = min(int(sizes[active].max()) + t, int(cur.shape[2]))
                cur = cur[:, :, :S_t].contiguous()                       # the longest slot of this step
                A_t, B_t = int(cur.shape[0]), int(cur.shape[1])
                K = min(B, B_t * n)
                res = _grow_step(model, cur, lo, n, K, min_gap, width, exclude, chunk_rows, act, counters)
                idx = active.to(dev)
                for key in ("rows", "logit", "proba", "parent", "added"):
                    out[key][idx, t, :K] = res[key]
                out["count"][idx, t] = res["count"]
                cur = res["beam"]
                n_cand += A_t * B_t * n
                n_steps += 1
        # the bins of every hub of a seed's last level, gathered back through parent
        last = (steps - 1).to(dev)                                       # -1: no level
        slot = torch.arange(B, device=dev).view(1, -1).expand(A, B).contiguous()
        for t in range(T - 1, -1, -1):
            on = (last >= t).view(-1, 1)
            out["path"][:, :, t] = torch.where(on, out["added"][:, t].gather(1, slot), out["path"][:, :, t])
            slot = torch.where(on, out["parent"][:, t].gather(1, slot), slot)
        final = out["count"].gather(1, last.clamp(min=0).view(-1, 1)) if T else zl(A, 1)
        live = (torch.arange(B, device=dev).view(1, -1) < final) & (last >= 0).view(-1, 1)
        out["path"] = torch.where(live.view(A, B, 1), out["path"], torch.zeros_like(out["path"]))
    c = counters.tolist()
    out.update(n_candidates=n_cand, n_invalid=c[0], n_twins=c[1], n_excluded=c[2], steps=n_steps)
    return out


# ---- multi-region sweep: candidates with bins drawn from several regions ------------------------------------------
MAX_PARTS = 8


def _region_parts(parts, min_gap: int):
    """(lo [P], n [P], m [P], C [P], k) of a validated part list; every refusal is a ValueError."""
    try:
        parts = [(int(lo), int(hi), int(m)) for lo, hi, m in parts]
    except (TypeError, ValueError):
        raise ValueError("parts must be a sequence of (lo, hi, m)")
    min_gap = int(min_gap)
    if not 1 <= len(parts) <= MAX_PARTS:
        raise ValueError(f"need 1 to {MAX_PARTS} parts (got {len(parts)})")
    if min_gap < 1:
        raise ValueError(f"need min_gap >= 1 (min_gap={min_gap})")
    for p, (lo, hi, m) in enumerate(parts):
        if m < 1 or hi - lo < 1 or hi - lo >= 1 << 31:
            raise ValueError(f"part {p}: need a region of 1 <= hi - lo < 2^31 bins and m >= 1 bins drawn from it (lo={lo} hi={hi} m={m})")
        if not 0 <= lo <= 1 << 62:
            raise ValueError(f"part {p}: lo out of range (lo={lo})")
        if p and parts[p - 1][1] > lo:
            raise ValueError(f"the regions must be ascending and disjoint: part {p} begins at {lo}, part {p - 1} ends at {parts[p - 1][1]}")
    k = sum(m for _, _, m in parts)
    if not 2 <= k <= _lib.MAX_L:
        raise ValueError(f"need 2 <= k <= {_lib.MAX_L} bins per candidate (k={k})")
    counts = [_free_count(hi - lo, m, min_gap) for lo, hi, m in parts]
    return [lo for lo, _, _ in parts], [hi - lo for lo, hi, _ in parts], [m for _, _, m in parts], counts, k


def region_count(parts, min_gap: int) -> int:
    """Number of candidates of a multi-region sweep: T = prod C_p with C_p = C(n_p - (m_p - 1)(min_gap - 1), m_p).  ``parts`` is a
    sequence of (lo, hi, m), 1 to 8 of them: m >= 1 bins drawn from the region [lo, hi) of node ids; the regions ascending and pairwise
    disjoint, 2 <= sum m <= 8.  A total >= 2^63 is refused (ValueError), not truncated."""
    _, _, _, counts, _ = _region_parts(parts, min_gap)
    total = math.prod(counts)
    if total >= 1 << 63:
        raise ValueError(f"{total} candidates (parts={list(parts)} min_gap={min_gap}) do not fit 63 bits")
    return total


def region_unrank(rank: int, parts, min_gap: int) -> Tuple[Tuple[int, ...], bool]:
    """(row, valid) of the candidate of global rank ``rank``, in Python integers (no GPU): how a rank is decoded, and the checker of the
    kernel.  The rank is the mixed radix ((r_0 C_1 + r_1) C_2 + ...) C_{P-1} + r_{P-1} of the parts' own lexicographic ranks; the row is
    the parts' candidates one behind the other, ascending as it stands.  It is valid iff every adjacent difference is >= min_gap, which
    can only fail between the last bin of one part and the first of the next."""
    los, ns, ms, counts, _ = _region_parts(parts, min_gap)
    rank, min_gap = _checked_rank(rank, region_count(parts, min_gap)), int(min_gap)
    pieces = []
    for p in range(len(los) - 1, -1, -1):
        rank, r = divmod(rank, counts[p])
        pieces.append(_subset_unrank(r, los[p], ns[p], ms[p], min_gap))
    row = tuple(v for piece in reversed(pieces) for v in piece)
    return row, all(b - a >= min_gap for a, b in zip(row, row[1:]))


def _part_arrays(los, ns, ms):
    P = len(los)
    return (C.c_int64 * P)(*los), (C.c_int32 * P)(*ns), (C.c_int32 * P)(*ms)


def region_rows(parts, min_gap: int, rank0: int = 0, count: Optional[int] = None, ranks: Optional[torch.Tensor] = None,
                width: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None,
                flag_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x int64 [count, width], flag int32 [count]) on the device: the candidates of the global ranks rank0 .. rank0 + count - 1, or of
    the device list ``ranks`` (a rank outside [0, T) gives an all-zero row with its flag set); flag != 0 marks an invalid candidate
    (region_unrank's rule).  Columns k .. width - 1 are zero (k <= width <= 8).  ``out`` / ``flag_out`` reuse buffers of at least
    count * width / count elements."""
    lib = _lib.load()
    los, ns, ms, _, k = _region_parts(parts, min_gap)
    total = region_count(parts, min_gap)
    min_gap = int(min_gap)
    width = _check_width(k, width)
    if ranks is not None:
        ranks = ranks.to(device=device, dtype=torch.long).contiguous().view(-1)
        device = ranks.device
    count = _rank_range(total, rank0, count, ranks)
    x, flag = _row_buffers(count, width, device if out is None else out.device, out, flag_out, "region_rows")
    if not x.is_cuda:
        raise _lib.MatchaHipError("region_rows needs a cuda device (no CPU fallback)")
    arrays = _part_arrays(los, ns, ms)                                   # host arrays, alive until the call returns: it reads them before
    lo_a, n_a, m_a = (C.cast(a, C.c_void_p) for a in arrays)
    with torch.cuda.device(x.device):
        _lib.check(lib.matcha_kway_region_rows(len(los), lo_a, n_a, m_a, min_gap, int(rank0), _lib.ptr(ranks), count, width, _lib.ptr(x),
                                               _lib.ptr(flag), _stream(x.device)), "matcha_kway_region_rows")
    return x, flag


def region_sweep(model, parts, min_gap: int, top: int, chunk_rows: int = 1 << 20, width: Optional[int] = None, exclude=None,
                 task_mode: str = "class", per_leading: bool = False) -> dict:
    """Score every candidate of a multi-region sweep (``parts``: (lo, hi, m) per region, see region_count) and keep the ``top`` best.

    Returns ``rows`` int64 [K', width], ``logit`` and ``proba`` [K'], ``rank`` int64 [K'] (the global rank; decode one with
    region_unrank), on the model's device and best first, and the integers ``n_candidates`` = T, ``n_invalid`` (candidates that break
    the gap rule across a part boundary; they are scored but never kept) and ``n_excluded`` (valid candidates found in ``exclude``).

    ``per_leading=True`` (needs two parts or more) keeps the best ``top`` PER CANDIDATE OF THE LEADING PART instead: with A = C_0 and
    K = min(top, T / C_0) it returns ``rows`` [A, K, width], ``logit``, ``proba`` and ``rank`` [A, K], ``count`` int64 [A] and
    ``leading`` int64 [A, m_0], the leading part's candidates in rank order; beyond count[a] the rank is -1 and rows, logit and proba
    are 0.  With m_0 = 1 that is, for every bin of the first region, its best hubs with partners in all the others.  An empty sweep
    (T = 0) returns A = 0.

    Eval mode and the loop (see the module's docstring) with region_rows and TopK.update or SegTopK.update: nothing synchronises until
    the end, where the node-id check of the whole sweep is raised once (IndexError)."""
    act = _activation(task_mode)
    los, ns, ms, counts, k = _region_parts(parts, min_gap)
    parts = [(lo, lo + n, m) for lo, n, m in zip(los, ns, ms)]
    min_gap, top, chunk_rows = int(min_gap), int(top), int(chunk_rows)
    width = _check_sweep_args(k, width, chunk_rows, top)
    if per_leading and len(parts) < 2:
        raise ValueError("per_leading needs at least two parts")
    total = region_count(parts, min_gap)
    model.eval()
    dev = model.layer_norm1.weight.device
    if total == 0:
        e = torch.empty(0, dtype=torch.float32, device=dev)
        out = {"rows": torch.empty(0, width, dtype=torch.long, device=dev), "logit": e, "proba": e.clone(),
               "rank": torch.empty(0, dtype=torch.long, device=dev), "n_candidates": 0, "n_invalid": 0, "n_excluded": 0}
        if per_leading:
            out.update(rows=out["rows"].view(0, 0, width), logit=e.view(0, 0), proba=e.clone().view(0, 0), rank=out["rank"].view(0, 0),
                       count=torch.empty(0, dtype=torch.long, device=dev), leading=torch.empty(0, ms[0], dtype=torch.long, device=dev))
        return out
    chunk_rows = min(chunk_rows, total)
    if per_leading:
        A, seg_len = counts[0], total // counts[0]
        K = min(top, seg_len)
        sel = SegTopK(A, K, seg_len, chunk_rows, dev)
    else:
        sel = TopK(min(top, total), chunk_rows, dev)
    tally = _tally(dev, "n_invalid", "n_excluded")
    rows = lambda g0, count, buf, fbuf: region_rows(parts, min_gap, rank0=g0, count=count, width=width, out=buf, flag_out=fbuf)
    with _pinned(model):
        for g0, _, logits, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev), rows, exclude, tally):
            sel.update(logits, g0, skip)
    if not per_leading:
        logit, rank = sel.result()
        rows, _ = region_rows(parts, min_gap, ranks=rank, width=width, device=dev)
        return {"rows": rows, "logit": logit, "proba": act(logit), "rank": rank, "n_candidates": total, **_counted(tally)}
    logit, rank, count = sel.read()
    rows, _ = region_rows(parts, min_gap, ranks=rank, width=width, device=dev)
    if ms[0] == 1:
        leading = torch.arange(los[0], los[0] + ns[0], dtype=torch.long, device=dev).view(-1, 1)
    else:                                                                # the first candidate of every segment begins with it
        first = torch.arange(A, dtype=torch.long, device=dev) * seg_len
        leading = region_rows(parts, min_gap, ranks=first, device=dev)[0][:, :ms[0]].contiguous()
    proba = torch.where(rank >= 0, act(logit), torch.zeros_like(logit))
    return {"rows": rows.view(A, K, width), "logit": logit, "proba": proba, "rank": rank, "count": count, "leading": leading,
            "n_candidates": total, **_counted(tally)}


def region_map_bound(parts, min_gap: int, rows_part: int, cols_part: int) -> int:
    """An upper bound, certainly not too small, on the candidates of a multi-region sweep that pass through one cell of region_map's
    pair map: rectangular (rows_part != cols_part), prod_{p not in {r, c}} C_p * C(n_r - 1, m_r - 1) * C(n_c - 1, m_c - 1) -- one bin of
    each of the two parts is fixed, the others are counted without the gap rule; symmetric, prod_{p != r} C_p * C(n_r - 2, m_r - 2)."""
    _, ns, ms, counts, _ = _region_parts(parts, min_gap)
    r, c = int(rows_part), int(cols_part)
    others = math.prod(cp for p, cp in enumerate(counts) if p not in (r, c))
    if r != c:
        return others * math.comb(ns[r] - 1, ms[r] - 1) * math.comb(ns[c] - 1, ms[c] - 1)
    return others * math.comb(ns[r] - 2, ms[r] - 2)


def region_map(model, parts, min_gap: int, rows_part: int, cols_part: int, chunk_rows: Optional[int] = 1 << 20, width: Optional[int] = None,
               exclude=None, task_mode: str = "class", threshold: float = 0.5, planes="all", value_max: Optional[float] = None) -> dict:
    """Score every candidate of a multi-region sweep (region_sweep's candidates, in its order, through the same loop) and project the
    probabilities onto pairs of bins, as kway_map does.  ``rows_part`` != ``cols_part`` (indices into ``parts``) gives the rectangular
    map [n_r, n_c] between the bins of two parts -- with parts on two chromosomes, the inter-chromosomal pair map; ``rows_part`` ==
    ``cols_part`` (a part with m >= 2) gives the symmetric map over that part's region (mirrored, zero diagonal).  Invalid candidates and
    the members of ``exclude`` contribute nothing.  Values, ``value_max``, ``threshold`` and ``planes`` as in kway_map; a sweep whose
    bound per cell (region_map_bound) times the largest value reaches 2^31 is refused before anything is launched.  The planes do not
    depend on ``chunk_rows`` (None: one chunk), bit for bit.

    Returns the planes (device tensors) and the integers ``n_candidates``, ``n_invalid``, ``n_excluded`` and ``n_rejected``."""
    act = _activation(task_mode)
    los, ns, ms, counts, k = _region_parts(parts, min_gap)
    parts = [(lo, lo + n, m) for lo, n, m in zip(los, ns, ms)]
    min_gap = int(min_gap)
    width = _check_width(k, width)
    total = region_count(parts, min_gap)
    chunk_rows = max(total, 1) if chunk_rows is None else int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1")
    r, c = int(rows_part), int(cols_part)
    if not (0 <= r < len(parts) and 0 <= c < len(parts)):
        raise ValueError(f"rows_part and cols_part must be indices into the {len(parts)} parts")
    if r == c and ms[r] < 2:
        raise ValueError(f"a symmetric map over part {r} needs at least two bins drawn from it (m={ms[r]})")
    if task_mode == "regress":
        if value_max is None:
            raise ValueError("task_mode 'regress' needs value_max: the largest value a candidate may contribute")
        vmax = float(value_max)
    else:
        vmax = 1.0
    if not 0.0 < vmax <= float(1 << 20):
        raise ValueError("value_max must be in (0, 2^20]")
    mask = _plane_mask(planes)
    bound = region_map_bound(parts, min_gap, r, c)
    if bound * vmax >= float(1 << 31):
        raise ValueError(f"a cell may receive {bound} candidates of value <= {vmax}: the sum's capacity of 2^31 per cell is not enough "
                         "(sweep smaller regions)")
    model.eval()
    dev = model.layer_norm1.weight.device
    if total == 0:
        out = _empty_map(ns[r], ns[c], mask, dev)
        if r != c and "max" in out:
            out["max"].fill_(float("-inf"))                              # a rectangular map has no diagonal
        out.update(n_candidates=0, n_invalid=0, n_excluded=0, n_rejected=0)
        return out
    chunk_rows = min(chunk_rows, total, (1 << 31) - 1)
    pm = PairMap((los[r], ns[r]), (los[c], ns[c]), mask, vmax=vmax, threshold=threshold, device=dev)
    tally = _tally(dev, "n_invalid", "n_excluded")
    rows = lambda g0, count, buf, fbuf: region_rows(parts, min_gap, rank0=g0, count=count, width=width, out=buf, flag_out=fbuf)
    value = lambda g0, x: act(model(x).reshape(-1))                      # a map takes values, not logits
    with _pinned(model):
        for _, x, v, skip, _ in _chunks(model, total, chunk_rows, _buffers(chunk_rows, width, dev), rows, exclude, tally, value):
            pm.update(x, v, skip)
    out = pm.result()
    out.pop("n_rows")
    out.update(n_candidates=total, **_counted(tally), n_rejected=int(out["n_rejected"].item()))
    return out
