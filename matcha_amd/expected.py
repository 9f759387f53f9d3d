"""Distance-matched expectation of k-way sweeps (csrc/expected.hip): observed over expected for k >= 3.

The classifier's raw logit is dominated by genomic distance: the training data holds mostly short-range clusters, so the best triples of
a chromosome are triples of neighbouring bins.  Hi-C tools judge a contact against the mean of all contacts at the same separation;
here a candidate of size k is judged against the mean of all candidates whose k - 1 gaps fall into the same classes -- its STRATUM.
The candidates of a sweep are never materialised, so the expectation is accumulated where they are made and scored, on the device:

    strata = GapStrata(k, edges)                     # the definition: gaps -> classes -> stratum
    stats  = GapStats(strata); stats.update(x, v)    # count / sum / sum of squares per stratum, int64 fixed point, any row order
    exp    = kway_expected(model, regions, k, gap)   # a sweep's loop around it: a GapExpected (save / load / table)
    out    = kway_enriched_sweep(model, lo, hi, k, gap, top)     # the best K by enrichment instead of by raw logit

``kway_map(..., expected=exp)`` (matcha_amd/sweep.py) is the observed-over-expected pair map.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import sweep as SW

MODES = ("logodds", "ratio", "z")
_PLANE_ORDER = ("count", "sum", "sumsq")


def default_gap_edges(n_max: int, k: int) -> Tuple[int, ...]:
    """The powers of two 2, 4, 8, ... below ``n_max``; the largest are dropped until (len + 1)^(k - 1) <= 2^20."""
    n_max, k = int(n_max), int(k)
    if not 2 <= k <= _lib.MAX_L:
        raise ValueError(f"k must be in [2, {_lib.MAX_L}]")
    edges = []
    e = 2
    while e < n_max and len(edges) < _lib.GAP_MAX_EDGES:
        edges.append(e)
        e *= 2
    while (len(edges) + 1) ** (k - 1) > _lib.GAP_MAX_STRATA:
        edges.pop()
    return tuple(edges)


class GapStrata:
    """The stratum of a candidate: ``edges``, a strictly ascending list of 0 to 15 positive integers, cuts the gaps g_j = x[j+1] - x[j]
    of a strictly ascending k-tuple of positive ids into G = len(edges) + 1 classes (class = the number of edges <= g), and the
    stratum is the classes read as a number in base G, first gap first: n_strata = G^(k-1) <= 2^20.  Mirror images keep their own
    strata."""

    def __init__(self, k: int, edges: Sequence[int] = ()):
        self.k = int(k)
        self.edges = tuple(int(e) for e in edges)
        if not 2 <= self.k <= _lib.MAX_L:
            raise ValueError(f"k must be in [2, {_lib.MAX_L}] (got {k})")
        if len(self.edges) > _lib.GAP_MAX_EDGES:
            raise ValueError(f"at most {_lib.GAP_MAX_EDGES} edges (got {len(self.edges)})")
        if any(e < 1 or e >= (1 << 63) - 1 for e in self.edges) or any(b <= a for a, b in zip(self.edges, self.edges[1:])):
            raise ValueError(f"edges must be positive and strictly ascending (got {list(self.edges)})")
        self.G = len(self.edges) + 1
        self.n_strata = self.G ** (self.k - 1)
        if self.n_strata > _lib.GAP_MAX_STRATA:
            raise ValueError(f"{self.G}^{self.k - 1} = {self.n_strata} strata exceed 2^20: use fewer edges (default_gap_edges)")
        self._edges_c = (C.c_int64 * max(len(self.edges), 1))(*self.edges)

    @property
    def edges_ptr(self):
        """The host array of the edges for the C ABI (kept alive by the object)."""
        return C.cast(self._edges_c, C.c_void_p) if self.edges else None

    def _rows(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 2 or x.dtype != torch.long or not x.is_cuda:
            raise ValueError("x must be an int64 [n, L] tensor on a cuda device (no CPU fallback)")
        if not self.k <= x.shape[1] <= _lib.MAX_L:
            raise ValueError(f"the row width must be in [k={self.k}, {_lib.MAX_L}] (got {x.shape[1]})")
        return x.contiguous()

    def ids(self, x: torch.Tensor) -> torch.Tensor:
        """int32 [n] on x's device: the stratum of every row of ``x`` int64 [n, L], -1 for a row that is no candidate of size k."""
        lib = _lib.load()
        x = self._rows(x)
        out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.matcha_gap_strata_ids(self.k, self.edges_ptr, len(self.edges), _lib.ptr(x), int(x.shape[0]), int(x.shape[1]), _lib.ptr(out),
                                                 SW._stream(x.device)), "matcha_gap_strata_ids")
        return out

    def enrich(self, x: torch.Tensor, score: torch.Tensor, offset: torch.Tensor, scale: torch.Tensor,
               want_strata: bool = False):
        """float32 [n]: (score - offset[s]) * scale[s] with s the row's stratum, rounded after each operation (numpy float32 arithmetic
        reproduces it bit for bit), NaN for a row without a stratum.  ``want_strata``: (enrichment, int32 strata)."""
        lib = _lib.load()
        x = self._rows(x)
        score = score.reshape(-1)
        for name, t, n in (("score", score, x.shape[0]), ("offset", offset, self.n_strata), ("scale", scale, self.n_strata)):
            if t.dtype != torch.float32 or t.device != x.device or t.numel() != n or t.dim() != 1:
                raise ValueError(f"{name} must be a float32 [{n}] tensor on x's device")
        score, offset, scale = score.contiguous(), offset.contiguous(), scale.contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        strata = torch.empty(x.shape[0], dtype=torch.int32, device=x.device) if want_strata else None
        with torch.cuda.device(x.device):
            _lib.check(lib.matcha_gap_enrich(self.k, self.edges_ptr, len(self.edges), _lib.ptr(x), int(x.shape[0]), int(x.shape[1]), _lib.ptr(score),
                                             _lib.ptr(offset), _lib.ptr(scale), _lib.ptr(strata), _lib.ptr(out), SW._stream(x.device)),
                       "matcha_gap_enrich")
        return (out, strata) if want_strata else out

    def decode(self, s: int) -> Tuple[Tuple[int, Optional[int]], ...]:
        """The gap ranges of stratum ``s``: per gap (lowest gap, highest gap or None for the open last class)."""
        s = int(s)
        if not 0 <= s < self.n_strata:
            raise IndexError(f"stratum {s} outside [0, {self.n_strata})")
        classes = []
        for _ in range(self.k - 1):
            classes.append(s % self.G)
            s //= self.G
        bounds = (1,) + self.edges
        return tuple((bounds[c], self.edges[c] - 1 if c < len(self.edges) else None) for c in reversed(classes))


def _gap_plane_mask(planes) -> int:
    if planes is None or planes == "all":
        return _lib.GAP_ALL
    if isinstance(planes, int):
        mask = int(planes)
    else:
        names = [planes] if isinstance(planes, str) else list(planes)
        unknown = [p for p in names if p not in _lib.GAP_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose among {_PLANE_ORDER}")
        mask = sum(_lib.GAP_PLANES[p] for p in set(names))
    if not 1 <= mask <= _lib.GAP_ALL:
        raise ValueError(f"the plane mask must be in [1, {_lib.GAP_ALL}] (got {mask})")
    return mask


class GapStats:
    """Statistics of a value per stratum, on the device: 'count', 'sum' and 'sumsq' planes (int64 [n_strata]; the sums in fixed point
    with ``shift`` fractional bits, 16 .. 32), accumulated with integer adds, so every plane is bit for bit the same whatever the order
    of the rows and however they were cut into updates.  ``vmax``: the largest value accepted, 0 < vmax <= 2^20 (with 'sumsq' one row's
    vmax^2 * 2^shift must stay within 2^62).  ``direct``: every add goes straight to global memory (the A/B switch of the block-level
    accumulation; same planes)."""

    def __init__(self, strata: GapStrata, planes="all", vmax: float = 1.0, shift: int = 32, device="cuda", direct: bool = False):
        lib = _lib.load()
        self.strata, self.planes, self.vmax, self.shift = strata, _gap_plane_mask(planes), float(vmax), int(shift)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatchaHipError("GapStats needs a cuda device (no CPU fallback)")
        if not 16 <= self.shift <= 32:
            raise ValueError(f"shift must be in [16, 32] (got {shift})")
        if not 0.0 < self.vmax <= float(1 << 20):
            raise ValueError(f"vmax must be in (0, 2^20] (got {vmax})")
        if self.planes & _lib.GAP_SUMSQ and self.vmax * self.vmax * 2.0 ** self.shift > 2.0 ** 62:
            raise ValueError(f"with 'sumsq' vmax^2 * 2^shift must stay within 2^62 (vmax={vmax} shift={shift}): use a smaller shift")
        self._update_mask = self.planes | (_lib.GAP_DIRECT if direct else 0)
        self._dims = (strata.k, len(strata.edges), self.planes)
        self.bytes = int(lib.matcha_gap_stats_bytes(*self._dims))
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_gap_stats_init(_lib.ptr(self.state), self.bytes, *self._dims, SW._stream(self.device)), "matcha_gap_stats_init")

    def update(self, x: torch.Tensor, value: torch.Tensor, skip: Optional[torch.Tensor] = None):
        """``x`` int64 [n, L] on the device (k <= L <= 8), ``value`` float32 [n], ``skip`` int32 / bool [n] (non-zero = the row
        contributes nothing and is not counted).  A row that is no candidate of size k, or whose value is NaN, negative or > vmax,
        is counted as rejected.  Enqueued on the current stream; nothing is read back."""
        lib = _lib.load()
        x = self.strata._rows(x)
        value, skip = SW._scores_and_skip(value, skip, self.state.device, "GapStats")
        if x.device != self.state.device or value.numel() != x.shape[0]:
            raise ValueError("x and value must be an int64 [n, L] and a float32 [n] tensor on the GapStats' device")
        st = self.strata
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_gap_stats_update(_lib.ptr(self.state), self.bytes, st.k, st.edges_ptr, len(st.edges), self._update_mask, self.shift,
                                                   self.vmax, _lib.ptr(x), int(x.shape[1]), _lib.ptr(value), _lib.ptr(skip), int(x.shape[0]),
                                                   SW._stream(self.device)), "matcha_gap_stats_update")

    def read(self) -> dict:
        """The planes present as they are kept (int64 [n_strata], on the device, no synchronisation) and 'counters' int64 [2] =
        (accepted rows, rejected rows)."""
        lib = _lib.load()
        n = self.strata.n_strata
        out = {name: torch.empty(n, dtype=torch.long, device=self.device) for name in _PLANE_ORDER if self.planes & _lib.GAP_PLANES[name]}
        counters = torch.empty(2, dtype=torch.long, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.matcha_gap_stats_read(_lib.ptr(self.state), self.bytes, *self._dims, _lib.ptr(out.get("count")), _lib.ptr(out.get("sum")),
                                                 _lib.ptr(out.get("sumsq")), _lib.ptr(counters), SW._stream(self.device)), "matcha_gap_stats_read")
        out["counters"] = counters
        return out

    def result(self) -> dict:
        """Host numpy arrays: 'count' int64 (when kept), 'mean' float64 = sum / 2^shift / count (with sum and count; 0 where count is 0),
        'var' float64 = sumsq / 2^shift / count - mean^2, not below 0 (with all three), and the integers 'n_rows' and 'n_rejected'.
        One synchronising read.  OverflowError when a stratum's count is so large that its sum may have wrapped."""
        raw = {key: t.cpu().numpy() for key, t in self.read().items()}
        return stats_result(raw, self.vmax, self.shift)


def stats_result(raw: dict, vmax: float, shift: int) -> dict:
    """GapStats.result's arithmetic on raw host planes (count / sum / sumsq int64 arrays, counters)."""
    out = {"n_rows": int(raw["counters"][0]), "n_rejected": int(raw["counters"][1])}
    count = raw.get("count")
    if count is not None:
        out["count"] = count
        worst = int(count.max()) if count.size else 0
        if worst * (max(vmax, vmax * vmax) * 2.0 ** shift) >= 2.0 ** 63:
            raise OverflowError(f"a stratum holds {worst} rows of value <= {vmax}: its fixed-point sum may have wrapped at shift={shift}; "
                                "accumulate with a smaller shift")
        if "sum" in raw:
            div = np.maximum(count, 1).astype(np.float64)
            mean = np.where(count > 0, raw["sum"].astype(np.float64) / 2.0 ** shift / div, 0.0)
            out["mean"] = mean
            if "sumsq" in raw:
                out["var"] = np.where(count > 0, np.maximum(raw["sumsq"].astype(np.float64) / 2.0 ** shift / div - mean * mean, 0.0), 0.0)
    return out


class GapExpected:
    """The expectation of a sweep per stratum: what ``kway_expected`` returns and ``kway_enriched_sweep`` / ``kway_map`` apply.  Host
    arrays ``count`` int64, ``mean`` and ``var`` float64 [n_strata] (var None without the 'sumsq' plane), the counters, and what it was
    made from (k, edges, min_gap, width, task_mode, regions).  ``raw``: the int64 planes count / sum / sumsq as they were accumulated
    (32 fractional bits unless ``shift`` said otherwise), where the object comes from kway_expected; None after ``load``."""

    def __init__(self, k, edges, min_gap, width, task_mode, regions, count, mean, var, n_rows, n_rejected):
        self.strata = GapStrata(k, edges)
        self.k, self.edges, self.min_gap, self.width, self.task_mode = self.strata.k, self.strata.edges, int(min_gap), int(width), str(task_mode)
        self.regions = tuple((int(a), int(b)) for a, b in regions)
        self.count = np.asarray(count, dtype=np.int64)
        self.mean = np.asarray(mean, dtype=np.float64)
        self.var = None if var is None else np.asarray(var, dtype=np.float64)
        self.n_rows, self.n_rejected = int(n_rows), int(n_rejected)
        self.raw = None                                                  # kway_expected leaves the int64 planes here (not saved)
        if self.count.shape != (self.strata.n_strata,) or self.mean.shape != self.count.shape or (self.var is not None and self.var.shape != self.count.shape):
            raise ValueError(f"count, mean and var must have {self.strata.n_strata} entries")

    def save(self, path):
        """One .npz (numbers and names only)."""
        with open(path, "wb") as f:
            np.savez(f, k=np.int64(self.k), edges=np.asarray(self.edges, dtype=np.int64), min_gap=np.int64(self.min_gap), width=np.int64(self.width),
                     task_mode=np.asarray(self.task_mode), regions=np.asarray(self.regions, dtype=np.int64).reshape(-1, 2), count=self.count,
                     mean=self.mean, var=np.zeros(0) if self.var is None else self.var, has_var=np.bool_(self.var is not None),
                     counters=np.asarray([self.n_rows, self.n_rejected], dtype=np.int64))

    @classmethod
    def load(cls, path) -> "GapExpected":
        z = np.load(path, allow_pickle=False)
        return cls(int(z["k"]), [int(e) for e in z["edges"]], int(z["min_gap"]), int(z["width"]), str(z["task_mode"]),
                   [tuple(r) for r in z["regions"].tolist()], z["count"], z["mean"], z["var"] if bool(z["has_var"]) else None,
                   int(z["counters"][0]), int(z["counters"][1]))

    def table_host(self, mode: str = "logodds", min_count: int = 30) -> Tuple[np.ndarray, np.ndarray]:
        """float32 (offset, scale) [n_strata] on the host: a candidate's enrichment is (score - offset[s]) * scale[s].

        'logodds' (scores are logits): offset = log(E) - log1p(-E) in float64, then rounded; scale 1.  'ratio' (scores are activated
        values): offset 0, scale 1 / E.  'z' (activated values): offset E, scale 1 / sd; needs the variance.  An undersampled stratum
        -- count < min_count, or E <= 0 (for 'logodds' also E >= 1), or sd = 0 for 'z' -- gets offset NaN, so its candidates' enrichment
        is NaN and TopK never keeps them."""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        if mode == "logodds" and self.task_mode == "regress":
            raise ValueError("mode 'logodds' needs probabilities: task_mode 'regress' takes 'ratio' or 'z'")
        if mode == "z" and self.var is None:
            raise ValueError("mode 'z' needs the 'sumsq' plane")
        E = self.mean
        ok = (self.count >= int(min_count)) & (self.count > 0) & (E > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            if mode == "logodds":
                ok &= E < 1
                safe = np.where(ok, E, 0.5)
                offset, scale = np.log(safe) - np.log1p(-safe), np.ones_like(E)
            elif mode == "ratio":
                offset, scale = np.zeros_like(E), 1.0 / np.where(ok, E, 1.0)
            else:
                sd = np.sqrt(self.var)
                ok &= sd > 0
                offset, scale = E.copy(), 1.0 / np.where(ok, sd, 1.0)
        offset = np.where(ok, offset, np.nan).astype(np.float32)
        scale = np.where(ok, scale, 1.0).astype(np.float32)
        return offset, scale

    def table(self, mode: str = "logodds", min_count: int = 30, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
        """``table_host`` on the device."""
        offset, scale = self.table_host(mode, min_count)
        return torch.from_numpy(offset).to(device), torch.from_numpy(scale).to(device)


def _expected_pass(model, strata, regions, k, min_gap, width, chunk_rows, act, vmax, shift, keep=None) -> GapStats:
    """The loop of matcha_amd/sweep.py with kway_rows and GapStats.update, over every region into one table and through one row
    buffer.  ``keep``: a float32 buffer that receives the logits of the (single) region in rank order."""
    dev = model.layer_norm1.weight.device
    stats = GapStats(strata, "all", vmax=vmax, shift=shift, device=dev)
    totals = [SW.kway_count(hi - lo, k, min_gap) if hi - lo >= 1 else 0 for lo, hi in regions]
    most = min(chunk_rows, max(totals + [0]))
    if most == 0:
        return stats
    buffers = SW._buffers(most, width, dev, flags=False)
    with SW._pinned(model):
        for (lo, hi), total in zip(regions, totals):
            rows = lambda r0, count, buf, _: SW.kway_rows(lo, hi - lo, k, min_gap, rank0=r0, count=count, width=width, out=buf)
            for r0, x, logits, _, _ in SW._chunks(model, total, most, buffers, rows, None, {}):
                if keep is not None:
                    keep[r0:r0 + logits.numel()] = logits
                stats.update(x, act(logits))
    return stats


def kway_expected(model, regions, k: int, min_gap: int, edges: Optional[Sequence[int]] = None, width: Optional[int] = None,
                  chunk_rows: int = 1 << 20, task_mode: str = "class", vmax: Optional[float] = None, shift: int = 32) -> GapExpected:
    """The expectation of the k-way candidates of ``regions`` (a list of (lo, hi) ranges of node ids): every candidate kway_sweep would
    score in each region is scored, and count, mean and variance of its value -- sigmoid(logit), or softplus(logit) for task_mode
    'regress', where ``vmax`` is required -- are accumulated per stratum of its gaps, all regions into ONE table: the stratum depends
    on gaps only, so a genome-wide expectation is the Hi-C convention.  Known hyperedges are part of the background and are included.
    ``edges``: default_gap_edges of the longest region.  Eval mode and the loop of matcha_amd/sweep.py (no grad, the large-batch route
    pinned, one reused rows buffer, nothing synchronises per chunk); the table does not depend on ``chunk_rows``, bit for bit."""
    act = SW._activation(task_mode)
    k, min_gap, chunk_rows = int(k), int(min_gap), int(chunk_rows)
    regions = [(int(lo), int(hi)) for lo, hi in regions]
    width = SW._check_sweep_args(k, width, chunk_rows)
    if task_mode == "regress" and vmax is None:
        raise ValueError("task_mode 'regress' needs vmax: the largest value a candidate may contribute")
    vmax = 1.0 if vmax is None else float(vmax)
    if edges is None:
        edges = default_gap_edges(max([hi - lo for lo, hi in regions] + [0]), k)
    strata = GapStrata(k, edges)
    for lo, hi in regions:
        if hi - lo >= 1:
            SW._check_args(hi - lo, k, min_gap)
    model.eval()
    stats = _expected_pass(model, strata, regions, k, min_gap, width, chunk_rows, act, vmax, int(shift))
    return _as_expected(stats, min_gap, width, task_mode, regions)


def _as_expected(stats: GapStats, min_gap, width, task_mode, regions) -> GapExpected:
    raw = {key: t.cpu().numpy() for key, t in stats.read().items()}
    r = stats_result(raw, stats.vmax, stats.shift)
    ex = GapExpected(stats.strata.k, stats.strata.edges, min_gap, width, task_mode, regions, r["count"], r["mean"], r["var"], r["n_rows"],
                     r["n_rejected"])
    ex.raw = {name: raw[name] for name in _PLANE_ORDER}
    return ex


def kway_enriched_sweep(model, lo: int, hi: int, k: int, min_gap: int, top: int, expected: Optional[GapExpected] = None, mode: str = "logodds",
                        min_count: int = 30, edges: Optional[Sequence[int]] = None, width: Optional[int] = None, exclude=None,
                        chunk_rows: int = 1 << 20, task_mode: str = "class", cache_rows: int = 1 << 26, vmax: Optional[float] = None) -> dict:
    """kway_sweep ranked by enrichment over the distance-matched expectation instead of by raw logit: the ``top`` candidates of [lo, hi)
    whose score lies furthest above what candidates of the same gap classes score on average.

    ``expected``: a GapExpected (kway_expected, or GapExpected.load); None computes the expectation of [lo, hi) itself first.  When that
    pass covers the same region and holds at most ``cache_rows`` candidates its logits stay on the device and the second forward is
    skipped -- the sweep pins the forward route, so the cached logits are the bits the second pass would produce.  ``mode``: 'logodds'
    (logit minus the logit of the stratum's mean probability), 'ratio' or 'z' (on the activated value; GapExpected.table_host).
    Candidates of strata with fewer than ``min_count`` candidates have no enrichment and are never kept (``n_undersampled``).
    ``exclude`` skips and counts known hyperedges in the ranking; the expectation still includes them.

    Returns kway_sweep's dictionary (rows, logit, proba, rank, best ENRICHMENT first, n_candidates, n_excluded) plus ``enrich`` [K'],
    ``stratum`` int32 [K'], ``expected`` [K'] (the stratum's mean, float64), ``n_undersampled`` and ``expected_table`` (the
    GapExpected)."""
    act = SW._activation(task_mode)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    if mode == "logodds" and task_mode == "regress":
        raise ValueError("mode 'logodds' needs probabilities: task_mode 'regress' takes 'ratio' or 'z'")
    lo, hi, k, min_gap, top, chunk_rows = int(lo), int(hi), int(k), int(min_gap), int(top), int(chunk_rows)
    n = hi - lo
    width = SW._check_sweep_args(k, width, chunk_rows, top)
    model.eval()
    dev = model.layer_norm1.weight.device
    total = SW.kway_count(n, k, min_gap) if n >= 1 else 0
    cache = None
    if expected is None:
        if task_mode == "regress" and vmax is None:
            raise ValueError("task_mode 'regress' needs vmax (or an expected table)")
        strata = GapStrata(k, default_gap_edges(n, k) if edges is None else edges)
        if 0 < total <= int(cache_rows):
            cache = torch.empty(total, dtype=torch.float32, device=dev)
        stats = _expected_pass(model, strata, [(lo, hi)], k, min_gap, width, chunk_rows, act, 1.0 if vmax is None else float(vmax), 32, keep=cache)
        expected = _as_expected(stats, min_gap, width, task_mode, [(lo, hi)])
    elif expected.k != k:
        raise ValueError(f"the expected table is for k={expected.k}, the sweep for k={k}")
    elif expected.task_mode != task_mode:
        raise ValueError(f"the expected table is for task_mode {expected.task_mode!r}, the sweep for {task_mode!r}")
    strata = expected.strata
    e = torch.empty(0, dtype=torch.float32, device=dev)
    if total == 0:
        return {"rows": torch.empty(0, width, dtype=torch.long, device=dev), "logit": e, "proba": e.clone(), "rank": torch.empty(0, dtype=torch.long, device=dev),
                "n_candidates": 0, "n_excluded": 0, "enrich": e.clone(), "stratum": torch.empty(0, dtype=torch.int32, device=dev),
                "expected": torch.empty(0, dtype=torch.float64, device=dev), "n_undersampled": 0, "expected_table": expected}
    offset, scale = expected.table(mode, min_count, device=dev)
    under = torch.isnan(offset)
    chunk_rows = min(chunk_rows, total)
    sel = SW.TopK(min(top, total), chunk_rows, dev)
    tally = SW._tally(dev, "n_excluded", "n_undersampled")
    rows = lambda r0, count, buf, _: SW.kway_rows(lo, n, k, min_gap, rank0=r0, count=count, width=width, out=buf)

    def enrichment(r0, x):                                               # what TopK ranks: from the cached logits, or the model's
        logits = cache[r0:r0 + x.shape[0]] if cache is not None else model(x).reshape(-1)
        enr, s = strata.enrich(x, logits if mode == "logodds" else act(logits), offset, scale, want_strata=True)
        tally["n_undersampled"] += under[s.long()].sum()                 # a sweep's rows all have a stratum
        return enr

    with SW._pinned(model):                                              # held across the winners' forward below: the same route
        for r0, _, enr, skip, _ in SW._chunks(model, total, chunk_rows, SW._buffers(chunk_rows, width, dev, flags=False), rows, exclude,
                                              tally, enrichment):
            sel.update(enr, r0, skip)
        enrich, rank = sel.result()
        if rank.numel():
            rows = SW.kway_rows(lo, n, k, min_gap, ranks=rank, width=width, device=dev)
        else:                                                            # every candidate undersampled or excluded
            rows = torch.empty(0, width, dtype=torch.long, device=dev)
        # the winners' logits: from the cache, or one more forward of K' rows on the sweep's pinned route (the same bits)
        if cache is not None:
            logit = cache[rank]
        else:
            logit = model(rows).reshape(-1) if rows.shape[0] else e
    stratum = strata.ids(rows) if rows.shape[0] else torch.empty(0, dtype=torch.int32, device=dev)
    mean = torch.from_numpy(expected.mean).to(dev)[stratum.long()]
    return {"rows": rows, "logit": logit, "proba": act(logit), "rank": rank, "n_candidates": total, **SW._counted(tally),
            "enrich": enrich, "stratum": stratum, "expected": mean, "expected_table": expected}
