"""Device-side negative sampling (reference main.py:361-459) over an exact hash set (utils.py:75-97 builds Bloom
filters; see matcha_amd/csrc/sampler.hip).  Thin wrappers over the C ABI; torch is used for memory only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _check_width(L: int, what: str):
    if L > _lib.MAX_LONG_L:          # (a width below 1 is refused by the library, as it always was)
        raise ValueError(f"{what}: rows of {L} columns (at most {_lib.MAX_LONG_L} are supported)")


class HyperedgeSet:
    """Exact membership set of known hyperedges (all sizes in one table).  ``edges``: int64 [M, L] zero-padded, L <= 32,
    each row ascending.  ``HyperedgeSet.empty(device, L)`` reproduces the reference's phase 1, where the
    "dict" is a list of empty python sets (main.py:589) and negatives come out equal to their positives.

    Routing: a set of width <= 8 is built, and asked about rows of width <= 8, through matcha_hashset_build / matcha_hashset_contains;
    when either width is 9 .. 32 the ``_long`` entry points are called.  The table has one format either way (a row's hash runs over
    its non-zero prefix), so a wide set answers narrow queries and a narrow set wide ones.  A width above 32 is a ValueError."""

    def __init__(self, edges: torch.Tensor):
        lib = _lib.load()
        if not edges.is_cuda:
            raise _lib.MatchaHipError("HyperedgeSet needs a cuda tensor (no CPU fallback)")
        _check_width(int(edges.shape[1]), "HyperedgeSet")
        self.edges = edges.to(torch.long).contiguous()
        self.n, self.L = int(self.edges.shape[0]), int(self.edges.shape[1])
        nbytes = lib.matcha_hashset_bytes(self.n)
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=edges.device)
        st = C.c_void_p(torch.cuda.current_stream(edges.device).cuda_stream)
        name = "matcha_hashset_build" if self.L <= _lib.MAX_L else "matcha_hashset_build_long"
        _lib.check(getattr(lib, name)(_lib.ptr(self.table), nbytes, _lib.ptr(self.edges), self.n, self.L, st), name)

    @classmethod
    def empty(cls, device, L: int):
        return cls(torch.zeros((0, L), dtype=torch.long, device=device))

    def contains(self, rows: torch.Tensor) -> torch.Tensor:
        """bool [n]: is row i of ``rows`` (int64 [n, L], L <= 32, zero-padded ascending) a known hyperedge."""
        lib = _lib.load()
        _check_width(int(rows.shape[1]), "HyperedgeSet.contains")
        rows = rows.to(device=self.edges.device, dtype=torch.long).contiguous()
        out = torch.empty(rows.shape[0], dtype=torch.int32, device=rows.device)
        st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
        name = "matcha_hashset_contains" if max(self.L, int(rows.shape[1])) <= _lib.MAX_L else "matcha_hashset_contains_long"
        _lib.check(getattr(lib, name)(_lib.ptr(self.table), _lib.ptr(self.edges), self.L, _lib.ptr(rows), rows.shape[0],
                                      rows.shape[1], _lib.ptr(out), st), name)
        return out.bool()


class NegativeSampler:
    """generate_negative (main.py:361-459): ``neg_num`` corrupted copies of every positive -- positions chosen with
    Binomial(k, 1/2) != 0 multiplicity, each replaced by a uniform bin of the SAME chromosome, redrawn until the row
    is duplicate-free, has all adjacent gaps > min_dis and is not a known hyperedge.

    Positives of up to 32 columns.  When the set and the positives are both at most 8 wide the call is matcha_neg_sample
    (neg_sample_kernel, one lane per negative); otherwise matcha_neg_sample_long (neg_sample_long_kernel, one lane per position), whose
    replacement counters are 32*trial + position above 8 columns.  A width above 32 is a ValueError before any launch."""

    def __init__(self, hset: HyperedgeSet, node2chrom: np.ndarray, chrom_range: np.ndarray, neg_num: int = 3, min_dis: int = 0,
                 seed: int = 0):
        dev = hset.edges.device
        self.hset, self.neg_num, self.min_dis = hset, int(neg_num), int(min_dis)
        self.node2chrom = torch.as_tensor(np.asarray(node2chrom, dtype=np.int32), device=dev)
        self.chrom_range = torch.as_tensor(np.asarray(chrom_range, dtype=np.int32), device=dev).contiguous()
        self.seed = torch.full((1,), int(seed), dtype=torch.int64, device=dev)
        self.n_nodes = int(self.node2chrom.numel()) - 1
        self.n_chrom = int(self.chrom_range.shape[0])
        # device status word (include/matcha_hip.h): [0] bit 1 = a node without a chromosome was met, [1] = negatives whose
        # trials were exhausted (returned equal to their positive); read it with check_status() at a point that syncs anyway
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)

    def sample_into(self, pos: torch.Tensor, neg_out: torch.Tensor, advance_seed: bool = True):
        """pos int64 [P,L] -> neg_out int64 [P*neg_num, L]; negatives of positive j at rows neg_num*j ... (main.py:383-428).
        Advances the seed on the device (graph-replay safe) unless the caller already did (``advance_seed=False``)."""
        lib = _lib.load()
        P, L = pos.shape
        _check_width(int(L), "NegativeSampler")
        st = C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream)
        if advance_seed:
            self.seed.add_(1)
        name = "matcha_neg_sample" if max(self.hset.L, int(L)) <= _lib.MAX_L else "matcha_neg_sample_long"
        _lib.check(getattr(lib, name)(_lib.ptr(self.hset.table), _lib.ptr(self.hset.edges), self.hset.n, self.hset.L, _lib.ptr(pos), P, L,
                                      self.neg_num, self.min_dis, _lib.ptr(self.node2chrom), self.n_nodes, _lib.ptr(self.chrom_range),
                                      self.n_chrom, _lib.ptr(self.seed), _lib.ptr(neg_out), _lib.ptr(self.status), st), name)
        return neg_out

    def check_status(self) -> int:
        """Synchronising read of the status word: raises KeyError if a node without a chromosome reached the sampler (the
        reference's ``chrom_range[node2chrom[node]]`` raises there, main.py:401-403); returns the number of negatives whose
        65 536 redraws were exhausted since the last call (the reference would still be looping, main.py:392)."""
        st = self.status.tolist()
        self.status.zero_()
        _lib.raise_on_status(st, "NegativeSampler")
        return int(st[1])

    def sample(self, pos: torch.Tensor) -> torch.Tensor:
        _check_width(int(pos.shape[1]), "NegativeSampler")
        pos = pos.to(torch.long).contiguous()
        out = torch.empty(pos.shape[0] * self.neg_num, pos.shape[1], dtype=torch.long, device=pos.device)
        return self.sample_into(pos, out)
