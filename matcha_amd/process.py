"""The reference's ``process.py`` up to the files the training flow reads: node dictionaries, the cluster
file -> ``edge_list.npy``, cooler pixels -> ``intra_adj.npy`` / ``inter_adj.npy``.

  build_node_dict   process.py:10-39    chrom sizes -> bin2node / node2bin / node2chrom / chrom_range (node ids from 1;
                                        ceil(size / res) + 1 bins per chromosome, as the reference's ``range(max_bin + 1)``)
  parse_clusters    process.py:42-87    SPRITE-style cluster file (id <tab> chr:pos <tab> ...) -> sorted unique node lists
  parse_clusters_device                 the same file -> the same clusters as (ids, offsets) device tensors, parsed on the device
                                        (csrc/cluster_text.hip); ``main(["--parse", "device"])``
  cool_index2node   process.py:121-137  cooler bin table -> node id per cooler bin (0 = not in chrom_list)
  pixels_to_adj     process.py:144-176  pixels -> intra / inter adjacency, accumulated on the device (csrc/features.hip)
  edgelist2adj      process.py:90-105   edge_list.npy -> edge_list_adj.npy, every cluster projected onto its pairs
  ClusterAdj / clusters_to_adj          the same projection as a stream: clusters -> intra / inter adjacency (or one matrix, with the
                                        History version's per-hyperedge weights and block-maximum normalisation, main_drop.py:543-563),
                                        accumulated on the device in int64 fixed point (csrc/cluster_adj.hip)

Reading the .mcool container itself (h5py) is out of scope: ``pixels_to_adj`` takes the arrays ``f['pixels']['bin1_id']``,
``['bin2_id']`` and ``['balanced']`` / ``['count']`` hold, in chunks of any size.  ``main(["--adj-from", "clusters"])`` needs no container:
the adjacency comes from the cluster file.
"""
from __future__ import annotations

import ctypes as C
import io
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def build_node_dict(chrom_size_path: str, chrom_list: Sequence[str], res: int, temp_dir: Optional[str] = None):
    """process.py:10-39.  The size file is tab-separated ``chrom <tab> size`` without a header; a chromosome listed twice
    takes its largest size (:22).  Returns (bin2node, node2bin, node2chrom, chrom_range int64 [C, 2]) and, with ``temp_dir``,
    writes the four .npy files the rest of the flow loads."""
    sizes: Dict[str, int] = {}
    with open(chrom_size_path) as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            if len(parts) < 2 or not parts[0]:
                continue
            sizes[parts[0]] = max(sizes.get(parts[0], 0), int(parts[1]))
    bin2node, node2bin, node2chrom, chrom_range = {}, {}, {}, []
    count = 1
    for j, chrom in enumerate(chrom_list):
        if chrom not in sizes:
            raise ValueError("%s is not in %s" % (chrom, chrom_size_path))      # the reference: np.max of an empty selection
        max_bin = math.ceil(sizes[chrom] / res)
        start = count
        for i in range(max_bin + 1):
            b = "%s:%d" % (chrom, i * res)
            bin2node[b] = count
            node2bin[count] = b
            node2chrom[count] = j
            count += 1
        chrom_range.append([start, count])
    chrom_range = np.asarray(chrom_range)
    if temp_dir is not None:
        os.makedirs(temp_dir, exist_ok=True)
        np.save(os.path.join(temp_dir, "chrom_range.npy"), chrom_range)
        np.save(os.path.join(temp_dir, "bin2node.npy"), bin2node)
        np.save(os.path.join(temp_dir, "node2chrom.npy"), node2chrom)
        np.save(os.path.join(temp_dir, "node2bin.npy"), node2bin)
    return bin2node, node2bin, node2chrom, chrom_range


def parse_clusters(cluster_path: str, bin2node: Dict[str, int], chrom_list: Sequence[str], res: int, max_cluster_size: int,
                   temp_dir: Optional[str] = None) -> List[List[int]]:
    """process.py:42-87: the first column is the cluster id; lines with fewer than 2 or more than 50 * max_cluster_size items
    are skipped before parsing, items of other chromosomes are dropped, positions are floored to their bin, node ids are
    de-duplicated; clusters with more than max_cluster_size or fewer than 2 nodes are dropped; sorted ascending."""
    final = []
    chrom_set = set(chrom_list)
    with open(cluster_path, "r") as f:
        for line in f:
            info_list = line.strip().split("\t")[1:]
            if len(info_list) < 2 or len(info_list) > max_cluster_size * 50:
                continue
            temp = []
            for info in info_list:
                try:
                    chrom, bin_ = info.split(":")
                except ValueError:
                    raise EOFError(info)
                if chrom not in chrom_set:
                    continue
                b = int(math.floor(int(bin_) / res)) * res
                temp.append(bin2node["%s:%d" % (chrom, b)])
            temp = sorted(set(temp))
            if len(temp) > max_cluster_size:
                continue
            if len(temp) > 1:
                final.append(temp)
    if temp_dir is not None:
        arr = np.empty(len(final), dtype=object)
        for i, c in enumerate(final):
            arr[i] = c
        np.save(os.path.join(temp_dir, "edge_list.npy"), arr, allow_pickle=True)
    return final


# ---- the cluster file parsed on the device ------------------------------------------------------------------------------
CLUSTER_NAME_MAX = _lib.CLUSTER_TEXT_NAME_MAX          # bytes per chromosome name in the device table
CLUSTER_CHROM_MAX = _lib.CLUSTER_TEXT_CHROM_MAX        # names the table holds
_STRIP_BYTES = bytes(range(0x09, 0x0e)) + bytes(range(0x1c, 0x21))      # what str.strip() removes from ASCII text


def cluster_chrom_table(chrom_list: Sequence[str], chrom_range, res: int):
    """The device parser's chromosome table from ``chrom_list`` and ``chrom_range`` (int [C, 2], ``[start, end)`` node ids as
    ``build_node_dict`` writes them): (names uint8 [C, 32] zero-padded, first_node int32 [C], n_bins int32 [C], n_nodes).  ValueError for
    what the table cannot hold: a duplicate, empty or non-ASCII name, a name with a blank, a control byte or a colon, a name longer than
    32 bytes, more than 256 names, a resolution outside 1 .. 2^31 - 1, a chromosome of more than 2^53 / res bins."""
    names = list(chrom_list)
    cr = np.asarray(chrom_range, dtype=np.int64).reshape(-1, 2)
    if len(cr) != len(names):
        raise ValueError("%d chromosome names for %d rows of chrom_range" % (len(names), len(cr)))
    if not 1 <= len(names) <= CLUSTER_CHROM_MAX:
        raise ValueError("the device parser's table holds 1 .. %d chromosome names, not %d" % (CLUSTER_CHROM_MAX, len(names)))
    if isinstance(res, bool) or int(res) != res or not 1 <= int(res) < (1 << 31):
        raise ValueError("res must be an integer in 1 .. 2^31 - 1, not %r" % (res,))
    res = int(res)
    table = np.zeros((len(names), CLUSTER_NAME_MAX), dtype=np.uint8)
    seen = set()
    for c, name in enumerate(names):
        if not isinstance(name, str):
            raise ValueError("chromosome name %r is not a string" % (name,))
        try:
            raw = name.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("chromosome name %r is not ASCII" % (name,))
        if not raw:
            raise ValueError("chromosome name %d is empty" % c)
        if any(b <= 0x20 or b == 0x3a for b in raw):
            raise ValueError("chromosome name %r holds a blank, a tab, a control byte or a colon" % (name,))
        if len(raw) > CLUSTER_NAME_MAX:
            raise ValueError("chromosome name %r is longer than %d bytes" % (name, CLUSTER_NAME_MAX))
        if raw in seen:
            raise ValueError("chromosome name %r is listed twice" % (name,))
        seen.add(raw)
        table[c, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    first, bins = cr[:, 0], cr[:, 1] - cr[:, 0]
    n_nodes = int(cr.max()) - 1
    if (first < 1).any() or (bins < 1).any() or n_nodes >= (1 << 31) - 1:
        raise ValueError("chrom_range rows must be [start, end) with 1 <= start < end < 2^31")
    if (bins > (1 << 53) // res).any():
        raise ValueError("a chromosome has more than 2^53 / res bins: its positions leave float64's integers")
    return table, np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(bins, dtype=np.int32), n_nodes


def _text_chunks(src, chunk_bytes: int):
    """Cut a cluster file (a path, or bytes) into runs of whole lines of at most ``chunk_bytes`` bytes: yields (file offset, buffer, length);
    ``buffer[:length]`` ends behind a ``\\r`` or ``\\n`` (found with ``rfind``) except at the end of the file, and is valid until the next
    chunk is asked for.  A line longer than ``chunk_bytes`` raises ValueError naming the byte offset it starts at."""
    chunk_bytes = int(chunk_bytes)
    if not 1 <= chunk_bytes < (1 << 31):
        raise ValueError("chunk_bytes must be in 1 .. 2^31 - 1, not %d" % chunk_bytes)
    if isinstance(src, (bytes, bytearray, memoryview)):
        f, total = io.BytesIO(src), len(src)
    else:
        f = open(os.fspath(src), "rb")
        total = os.fstat(f.fileno()).st_size
    with f:
        buf = bytearray(max(1, min(chunk_bytes, total)))
        view = memoryview(buf)
        base = have = 0                                                       # the file offset of buf[0]; bytes in buf
        while True:
            while have < len(buf):
                got = f.readinto(view[have:])
                if not got:
                    break
                have += got
            if have < len(buf):                                               # the end of the file: what is left is the last chunk
                if have:
                    yield base, buf, have
                return
            cut = max(buf.rfind(b"\n", 0, have), buf.rfind(b"\r", 0, have)) + 1
            if cut == 0:
                if f.read(1):
                    raise ValueError("the line at byte offset %d is longer than chunk_bytes = %d" % (base, chunk_bytes))
                yield base, buf, have                                         # the file ends with the buffer
                return
            yield base, buf, cut
            buf[:have - cut] = buf[cut:have]
            base, have = base + cut, have - cut


def _raise_cluster_text_error(st, base: int, buf, length: int):
    """The device status of one chunk as the exception the host parser raises for the FIRST offending item of the file."""
    if st[0] & _lib.CLUSTER_TEXT_ECOUNT:
        raise _lib.MatchaHipError("parse_clusters_device: the chunk's line and tab counts changed between the count and the parse")
    found = [(st[word], rank) for rank, (bit, word) in enumerate(((_lib.CLUSTER_TEXT_ESPLIT, 1), (_lib.CLUSTER_TEXT_EBIN, 2),
                                                                  (_lib.CLUSTER_TEXT_EGRAMMAR, 3), (_lib.CLUSTER_TEXT_ENONASCII, 4))) if st[0] & bit]
    off, rank = min(found)
    if rank == 3:
        raise ValueError("byte offset %d: byte 0x%02x is not ASCII (the device parser takes ASCII text only)" % (base + off, buf[off]))
    end = off
    while end < length and buf[end] not in b"\t\r\n":
        end += 1
    item = bytes(buf[off:end]).rstrip(_STRIP_BYTES).decode("ascii", "backslashreplace")
    where = "byte offset %d: item %r" % (base + off, item)
    if rank == 0:
        raise EOFError(where + " is not chrom:position")
    if rank == 1:
        raise KeyError(where + " lies past the last bin of its chromosome")
    raise ValueError(where + ": the position must be 1 to 18 ASCII digits")


def parse_clusters_device(cluster_path_or_bytes, chrom_list: Sequence[str], chrom_range, res: int, max_cluster_size: int,
                          chunk_bytes: int = 1 << 28, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """``parse_clusters`` on the device (csrc/cluster_text.hip): the cluster file (a path, or its bytes) -> the clusters in CSR
    form, (ids int32 [I], offsets int64 [M + 1]) device tensors, which ``ClusterAdj.update`` and ``kmers.generate_kmers`` take as they are.
    For every text it accepts, the CSR equals ``parse_clusters``'s lists bit for bit; an empty file, or one without a kept cluster, gives
    ids [0] and offsets [0].  The host reads the file in chunks of whole lines of at most ``chunk_bytes`` bytes.

    Errors keep the host parser's classes and name the byte offset and the text of the first offending item: EOFError for an item that is
    not ``chrom:position``, KeyError for a bin past its chromosome, ValueError for a position that is no number.  The grammar is narrower
    than ``int()``'s: a position is 1 to 18 ASCII digits (``+5``, `` 5``, ``2_500`` and ``-5`` are ValueError, 19 or more digits KeyError), and
    a byte >= 0x80 anywhere in the file is ValueError.  ``cluster_chrom_table`` lists what the chromosome table refuses.  There is no CPU
    path: without a GPU this raises MatchaHipError."""
    names, first, bins, n_nodes = cluster_chrom_table(chrom_list, chrom_range, res)
    max_cluster_size = int(max_cluster_size)
    if not 1 <= max_cluster_size <= (1 << 24):
        raise ValueError("max_cluster_size must be in 1 .. 2^24, not %d" % max_cluster_size)
    chunks = _text_chunks(cluster_path_or_bytes, chunk_bytes)
    chunk = next(chunks, None)                                                # a first line that is too long is refused here
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.MatchaHipError("parse_clusters_device needs a cuda device (no CPU fallback)")
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    i32, i64, u8 = (dict(dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.uint8))
    count_ws = torch.empty(lib.matcha_cluster_text_count_workspace_bytes(0), **u8)
    counts, n_out, status = torch.empty(2, **i64), torch.empty(2, **i64), torch.empty(8, **i32)
    ids_parts, off_parts, n_ids = [], [torch.zeros(1, **i64)], 0
    while chunk is not None:
        base, buf, length = chunk
        text = torch.frombuffer(buf, dtype=torch.uint8, count=length).to(dev)      # a copy from pageable memory: done when it returns
        _lib.check(lib.matcha_cluster_text_count(_lib.ptr(text), length, _lib.ptr(counts), _lib.ptr(count_ws), count_ws.numel(), st),
                   "matcha_cluster_text_count")
        n_lines, n_tabs = (int(v) for v in counts.tolist())                   # the chunk's one sizing sync
        ws_bytes = lib.matcha_cluster_text_workspace_bytes(length, n_lines, n_tabs)
        if ws_bytes == 0:
            raise _lib.MatchaHipError("matcha_cluster_text_workspace_bytes(%d, %d, %d) = 0" % (length, n_lines, n_tabs))
        ws = torch.empty(ws_bytes, **u8)
        ids, offsets = torch.empty(max(n_tabs, 1), **i32), torch.empty(n_lines + 1, **i64)
        _lib.check(lib.matcha_cluster_text_parse(_lib.ptr(text), length, n_lines, n_tabs, names.ctypes.data_as(C.c_void_p),
                                                 first.ctypes.data_as(C.c_void_p), bins.ctypes.data_as(C.c_void_p), len(first), int(res),
                                                 max_cluster_size, n_nodes, _lib.ptr(ids), ids.numel(), _lib.ptr(offsets), offsets.numel(),
                                                 _lib.ptr(n_out), C.c_void_p(n_out.data_ptr() + 8), _lib.ptr(status), _lib.ptr(ws), ws_bytes, st),
                   "matcha_cluster_text_parse")
        st_host = [int(v) for v in status.tolist()]
        if st_host[0]:
            _raise_cluster_text_error(st_host, base, buf, length)
        m, i = (int(v) for v in n_out.tolist())
        if m:
            ids_parts.append(ids[:i].clone())                                 # compact copies; the chunk's buffers are freed
            off_parts.append(offsets[1:m + 1] + n_ids)
            n_ids += i
        del ws, ids, offsets, text
        chunk = next(chunks, None)
    return (torch.cat(ids_parts) if ids_parts else torch.zeros(0, **i32)), torch.cat(off_parts)


def _is_device_csr(clusters) -> bool:
    return isinstance(clusters, tuple) and len(clusters) == 2 and isinstance(clusters[0], torch.Tensor) and clusters[0].device.type == "cuda"


def device_csr(clusters, device):
    """An (ids, offsets) pair whose ids are a device tensor -> (ids int32 on ``device``, never moved to the host; offsets int64 numpy, 8
    bytes per cluster, for what the callers compute on the host), checked like ``_clusters_csr`` checks a host pair."""
    ids, offsets = clusters
    offsets = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets), dtype=np.int64)
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != ids.numel() or ids.dim() != 1:
        raise ValueError("(ids, offsets): offsets must start at 0, not decrease and end at len(ids)")
    return ids.to(device=device, dtype=torch.int32).contiguous(), offsets


def cool_index2node(bins_chrom: np.ndarray, bins_start: np.ndarray, chrom_names: Sequence[str], chrom_list: Sequence[str],
                    bin2node: Dict[str, int]) -> np.ndarray:
    """process.py:121-137 as an int32 array: node id of every cooler bin, 0 for bins of chromosomes outside chrom_list.
    A bin of a listed chromosome that the node dictionary lacks raises KeyError, as the reference's dict lookup does."""
    names = [n.decode() if isinstance(n, bytes) else str(n) for n in chrom_names]
    listed = set(chrom_list)
    out = np.zeros(len(bins_chrom), dtype=np.int32)
    for i in range(len(bins_chrom)):
        chrom = names[int(bins_chrom[i])]
        if chrom in listed:
            out[i] = bin2node["%s:%d" % (chrom, int(bins_start[i]))]
    return out


def node2chrom_array(node2chrom: Dict[int, int], n_nodes: int) -> np.ndarray:
    out = np.full(n_nodes + 1, -1, dtype=np.int32)
    for k, v in node2chrom.items():
        if 0 < int(k) <= n_nodes:
            out[int(k)] = int(v)
    return out


def pixels_to_adj(bin1, bin2, count, index2node, node2chrom, n_nodes: int, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """process.py:144-172 on the device.  ``n_nodes`` = number of nodes N (the reference's matrices are
    [max(chrom_range) - 1]^2 = N x N, row = node id - 1).  Adds into ``out`` = (intra, inter) float64 [N, N] when given, so
    a large pixel table can be streamed through in chunks.  Each (bin1, bin2) of a cooler occurs once, so every cell receives
    one add (two on the diagonal) and the result does not depend on the order of the atomics."""
    lib = _lib.load()
    dev = torch.device(device)
    def dev_array(a, dtype):                               # numpy arrays, h5py datasets or tensors already on the device
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        return t.to(device=dev, dtype=dtype).contiguous()
    b1, b2 = dev_array(bin1, torch.int64), dev_array(bin2, torch.int64)
    cnt, i2n = dev_array(count, torch.float64), dev_array(index2node, torch.int32)
    n2c = node2chrom_array(node2chrom, n_nodes) if isinstance(node2chrom, dict) else np.asarray(node2chrom, dtype=np.int32)
    n2c = torch.from_numpy(n2c).to(dev)
    if len(n2c) < n_nodes + 1:
        raise ValueError("node2chrom must cover node ids 0 .. n_nodes")
    if out is None:
        out = (torch.zeros((n_nodes, n_nodes), dtype=torch.float64, device=dev), torch.zeros((n_nodes, n_nodes), dtype=torch.float64, device=dev))
    intra, inter = out
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.matcha_pixels_to_adj(_lib.ptr(b1), _lib.ptr(b2), _lib.ptr(cnt), b1.numel(), _lib.ptr(i2n), i2n.numel(), _lib.ptr(n2c),
                                        n_nodes, _lib.ptr(intra), _lib.ptr(inter), st), "matcha_pixels_to_adj")
    return intra, inter


# ---- contact matrices from the clusters ---------------------------------------------------------------------------------
MAX_ADJ_CLUSTER = 65535          # csrc/cluster_unrank.hpp kMaxClusterNodes: every local pair rank stays below 2^31
_Q_ONE = 1 << 32                 # the fixed point: q = rint(w 2^32)
_Q_SUM_LIMIT = 1 << 62           # bound on the running sum of |q|: a cell receives at most one add per cluster


def _clusters_csr(clusters):
    """(ids int32 [I], offsets int64 [M + 1]) from a list of id lists or from an (ids, offsets) TUPLE of two arrays / tensors."""
    if isinstance(clusters, tuple) and len(clusters) == 2 and all(isinstance(t, (np.ndarray, torch.Tensor)) for t in clusters):
        clusters = tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in clusters)
        ids = np.ascontiguousarray(np.asarray(clusters[0]), dtype=np.int32)
        offsets = np.ascontiguousarray(np.asarray(clusters[1]), dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != ids.size or ids.ndim != 1:
            raise ValueError("(ids, offsets): offsets must start at 0, not decrease and end at len(ids)")
        return ids, offsets
    lens = np.fromiter((len(c) for c in clusters), dtype=np.int64, count=len(clusters))
    offsets = np.zeros(len(clusters) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    ids = np.concatenate([np.asarray(c, dtype=np.int32).reshape(-1) for c in clusters]) if int(offsets[-1]) else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(ids, dtype=np.int32), offsets


def cluster_weights_q(lens: np.ndarray, weight) -> np.ndarray:
    """The clusters' fixed-point weights q = rint(w 2^32) as int64, computed in float64: ``"one"`` (edgelist2adj), ``"two_over_n"`` (2 / n for
    a cluster of n nodes) or one float per cluster (get_adjacency's ``weight``).  Weights must be finite and below 2^30 in magnitude."""
    lens = np.asarray(lens, dtype=np.int64)
    if isinstance(weight, str):
        if weight == "one":
            w = np.ones(len(lens), dtype=np.float64)
        elif weight == "two_over_n":
            w = 2.0 / np.maximum(lens, 1).astype(np.float64)
        else:
            raise ValueError("weight must be 'one', 'two_over_n' or an array, not %r" % (weight,))
    else:
        w = np.asarray(weight, dtype=np.float64).reshape(-1)
        if len(w) != len(lens):
            raise ValueError("%d weights for %d clusters" % (len(w), len(lens)))
    if not np.isfinite(w).all():
        raise ValueError("cluster weights must be finite")
    if len(w) and np.abs(w).max() >= float(1 << 30):
        raise ValueError("cluster weights must be below 2^30 in magnitude")
    return np.rint(w * float(_Q_ONE)).astype(np.int64)


class ClusterAdj:
    """Clusters -> contact matrices, accumulated on the device (csrc/cluster_adj.hip).  Every cluster adds its weight to every pair of its
    nodes, as the reference's ``edgelist2adj`` (process.py:90-105) and the History version's ``get_adjacency`` (main_drop.py:543-563) do; the
    sums are int64 in 2^-32 fixed point, so the matrices do not depend on the order of the clusters or on how they are cut into ``update``
    calls.  ``node2chrom``: the dict of ``build_node_dict`` or an int array [n_nodes + 1] (entry 0 unused); it may be None when only
    ``finish(split=False)`` is wanted.  There is no CPU path."""

    def __init__(self, n_nodes: int, node2chrom=None, device="cuda"):
        n_nodes = int(n_nodes)
        if n_nodes < 1:
            raise ValueError("n_nodes must be >= 1")
        self.n_nodes = n_nodes
        self.device = torch.device(device)
        if node2chrom is None:
            self._n2c_host = None
        else:
            n2c = node2chrom_array(node2chrom, n_nodes) if isinstance(node2chrom, dict) else np.asarray(node2chrom, dtype=np.int32)
            if len(n2c) < n_nodes + 1:
                raise ValueError("node2chrom must cover node ids 0 .. n_nodes")
            self._n2c_host = np.ascontiguousarray(n2c[:n_nodes + 1], dtype=np.int32)
        self.q_abs_sum = 0               # the running sum of |q| over every accepted update, a Python int
        self.n_pairs = 0
        self._acc = self._status = self._n2c = None

    def _state(self):
        if self._acc is None:
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise _lib.MatchaHipError("ClusterAdj needs a cuda device (no CPU fallback)")
            _lib.load()
            self._acc = torch.zeros((self.n_nodes, self.n_nodes), dtype=torch.int64, device=self.device)
            self._status = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._n2c = None if self._n2c_host is None else torch.from_numpy(self._n2c_host).to(self.device)
        return self._acc

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, clusters, weight="one"):
        """Add ``clusters`` (a list of ascending id lists, or an ``(ids, offsets)`` pair) with ``weight`` = "one" | "two_over_n" | one float per
        cluster.  A pair whose ids are a device tensor (``parse_clusters_device``) is used where it is: only its offsets are copied to the
        host.  Refused with ValueError before anything runs: a non-finite weight, a cluster of more than 65535 nodes, and an update that
        would take the running sum of |q| to 2^62.  Ids that are not strictly ascending or leave 1 .. n_nodes are found on the device: such a
        cluster adds nothing and ``status()[0]`` gets STATUS_BAD_ID."""
        lib = _lib.load()
        ids_d = None
        if _is_device_csr(clusters):                                          # ids stay where they are; offsets (8 bytes per cluster) come to the host
            ids_d, offsets = device_csr(clusters, self.device)
        else:
            ids, offsets = _clusters_csr(clusters)
        M = len(offsets) - 1
        lens = np.diff(offsets)
        q = cluster_weights_q(lens, weight)
        total = lib.matcha_cluster_pairs_count(offsets.ctypes.data_as(C.c_void_p), M)
        if total < 0:
            raise ValueError("a cluster has more than %d nodes (or the pair count leaves int63)" % MAX_ADJ_CLUSTER)
        q_sum = int(np.abs(q).astype(object).sum()) if M else 0
        if self.q_abs_sum + q_sum >= _Q_SUM_LIMIT:
            raise ValueError("the clusters' weights sum to %.6g or more: the fixed-point sums are bounded by 2^30"
                             % ((self.q_abs_sum + q_sum) / float(_Q_ONE)))
        acc = self._state()
        if M == 0 or total == 0:
            return self
        pair_ptr = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(lens * (lens - 1) // 2, out=pair_ptr[1:])
        dev = self.device
        if ids_d is None:
            ids_d = torch.from_numpy(ids).to(dev)
        off_d = torch.from_numpy(offsets).to(dev)
        q_d, ptr_d = torch.from_numpy(q).to(dev), torch.from_numpy(pair_ptr).to(dev)
        _lib.check(lib.matcha_cluster_adj_update(_lib.ptr(ids_d), _lib.ptr(off_d), _lib.ptr(q_d), _lib.ptr(ptr_d), M, self.n_nodes, _lib.ptr(acc),
                                                 _lib.ptr(self._status), self._stream()), "matcha_cluster_adj_update")
        self.q_abs_sum += q_sum
        self.n_pairs += int(total)
        return self

    def finish(self, split: bool = True):
        """(intra, inter) float64 [n_nodes, n_nodes] on the device, or with ``split=False`` the one matrix of ``edgelist2adj``.  Symmetric,
        zero diagonal; the accumulator is kept, so more updates may follow."""
        lib = _lib.load()
        acc = self._state()
        N = self.n_nodes
        intra = torch.empty((N, N), dtype=torch.float64, device=self.device)
        if split:
            if self._n2c is None:
                raise ValueError("finish(split=True) needs node2chrom")
            inter = torch.empty((N, N), dtype=torch.float64, device=self.device)
            _lib.check(lib.matcha_cluster_adj_finish(_lib.ptr(acc), _lib.ptr(self._n2c), N, _lib.ptr(intra), _lib.ptr(inter), self._stream()),
                       "matcha_cluster_adj_finish")
            return intra, inter
        _lib.check(lib.matcha_cluster_adj_finish(_lib.ptr(acc), None, N, _lib.ptr(intra), None, self._stream()), "matcha_cluster_adj_finish")
        return intra

    def status(self) -> List[int]:
        """The device status words as a list of 4 ints ([0] & STATUS_BAD_ID: a cluster was rejected)."""
        self._state()
        return [int(v) for v in self._status.cpu().tolist()]


def block_colmax_normalise_(A: torch.Tensor, ranges) -> torch.Tensor:
    """In place on the float64 device matrix A [N, N]: for every 0-based row block [lo, hi) of ``ranges`` [C, 2] and every column,
    A[lo:hi, col] /= A[lo:hi, col].max() + 1e-10 (main_drop.py:552-561)."""
    lib = _lib.load()
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float64 or not A.is_contiguous() or A.device.type != "cuda":
        raise _lib.MatchaHipError("block_colmax_normalise_ needs a contiguous square float64 matrix on a cuda device (no CPU fallback)")
    N = int(A.shape[0])
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
    if len(r) and ((r[:, 0] < 0).any() or (r[:, 1] > N).any() or (r[:, 0] > r[:, 1]).any()):
        raise ValueError("row blocks must satisfy 0 <= lo <= hi <= %d" % N)
    order = np.argsort(r[:, 0], kind="stable")
    if len(r) > 1 and (r[order][1:, 0] < r[order][:-1, 1]).any():
        raise ValueError("row blocks must not overlap")
    if len(r) == 0:
        return A
    r_d = torch.from_numpy(r).to(A.device)
    ws_bytes = lib.matcha_block_colmax_workspace_bytes(N, len(r))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=A.device)
    st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
    _lib.check(lib.matcha_block_colmax_normalise(_lib.ptr(A), N, _lib.ptr(r_d), len(r), _lib.ptr(ws), ws_bytes, st), "matcha_block_colmax_normalise")
    return A


def clusters_to_adj(clusters, node2chrom, n_nodes: int, weight="one", normalise: Optional[str] = None, chrom_range=None, split: bool = True,
                    device="cuda"):
    """One shot: ``ClusterAdj(n_nodes, node2chrom).update(clusters, weight).finish()`` -> (intra, inter) float64 on the device, or with
    ``split=False`` the one matrix.

    ``normalise="block_max"`` is the History version's ``get_adjacency(norm=True)``: every block of rows of ``chrom_range`` (int [C, 2],
    1-based node ids, ``[start, end)``, as ``build_node_dict`` writes it) is divided per column by its maximum + 1e-10.  It is applied to the
    single unsplit matrix, and the split (if asked for) is taken from the normalised matrix.

    Against the reference: ``edgelist2adj`` is ``weight="one", split=False`` on the same 1-based ids (its matrix row is id - 1, as here).
    ``get_adjacency(data, weight, norm)`` works on 0-based ids ``datum`` and on ``num`` (``nums_type``), the node count per type: pass the
    clusters as ``datum + 1``, ``weight`` as its per-hyperedge array, and ``chrom_range = [[1 + sum(num[:t]), 1 + sum(num[:t + 1])] for t]``;
    its result is this function's ``split=False`` matrix cast to float32 (it returns a float32 csr_matrix).  Integer weights are exact, so
    both are reproduced bit for bit; other weights are rounded once to 2^-32 and then summed exactly."""
    if normalise not in (None, "block_max"):
        raise ValueError("normalise must be None or 'block_max', not %r" % (normalise,))
    if normalise == "block_max" and chrom_range is None:
        raise ValueError("normalise='block_max' needs chrom_range")
    ca = ClusterAdj(n_nodes, node2chrom, device=device)
    ca.update(clusters, weight)
    if normalise is None:
        return ca.finish(split=split)
    A = ca.finish(split=False)
    block_colmax_normalise_(A, np.asarray(chrom_range, dtype=np.int64).reshape(-1, 2) - 1)
    if not split:
        return A
    if ca._n2c is None:
        raise ValueError("the split needs node2chrom")
    n2c = ca._n2c[1:].to(torch.int64)
    same = n2c[:, None] == n2c[None, :]
    zero = torch.zeros((), dtype=A.dtype, device=A.device)
    return torch.where(same, A, zero), torch.where(same, zero, A)


def edgelist2adj(temp_dir: str, device="cuda") -> np.ndarray:
    """process.py:90-105: ``edge_list.npy`` + ``chrom_range.npy`` -> ``edge_list_adj.npy``, float64 [N, N] with N = max(chrom_range) - 1."""
    edge_list = np.load(os.path.join(temp_dir, "edge_list.npy"), allow_pickle=True)
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy"), allow_pickle=True)
    N = int(np.max(chrom_range)) - 1
    adj = clusters_to_adj([list(e) for e in edge_list], None, N, weight="one", split=False, device=device).cpu().numpy()
    np.save(os.path.join(temp_dir, "edge_list_adj.npy"), adj)
    return adj


def save_adj(temp_dir: str, intra: torch.Tensor, inter: torch.Tensor):
    """process.py:175-176."""
    np.save(os.path.join(temp_dir, "intra_adj.npy"), intra.cpu().numpy())
    np.save(os.path.join(temp_dir, "inter_adj.npy"), inter.cpu().numpy())


def save_clusters_csr(temp_dir: str, clusters, edge_list_npy: bool = True):
    """``temp_dir/edge_list_csr.npz`` (``ids`` int32, ``offsets`` int64) from an (ids, offsets) pair, which ``kmers.main --clusters csr`` reads;
    with ``edge_list_npy`` also the reference's ``edge_list.npy``, the object array of id lists its other tools load."""
    ids, offsets = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in clusters)
    ids, offsets = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(offsets, dtype=np.int64)
    os.makedirs(temp_dir, exist_ok=True)
    np.savez(os.path.join(temp_dir, "edge_list_csr.npz"), ids=ids, offsets=offsets)
    if edge_list_npy:
        arr = np.empty(len(offsets) - 1, dtype=object)
        flat = ids.tolist()
        for i in range(len(arr)):
            arr[i] = flat[offsets[i]:offsets[i + 1]]
        np.save(os.path.join(temp_dir, "edge_list.npy"), arr, allow_pickle=True)


def main(argv=None):
    """The script body of process.py:229-242: node dictionaries, edge_list.npy and the adjacency matrices -- with ``--adj-from mcool`` (the
    default) from ``mcool_path`` when h5py is importable (it is not part of this image), streamed through the device 16 M pixels at a time;
    with ``--adj-from clusters`` from the cluster file itself (ClusterAdj), which needs no h5py."""
    import argparse
    import json
    ap = argparse.ArgumentParser(description="process.py on the MI355X path")
    ap.add_argument("--config", default="./config.JSON")
    ap.add_argument("--adj-from", choices=["mcool", "clusters"], default="mcool", help="where intra_adj.npy / inter_adj.npy come from")
    ap.add_argument("--adj-weight", choices=["one", "two_over_n"], default="one", help="--adj-from clusters: a cluster's weight per pair")
    ap.add_argument("--adj-max-cluster-size", type=int, default=None,
                    help="--adj-from clusters: largest cluster that enters the contact matrix (default: the config's max_cluster_size)")
    ap.add_argument("--parse", choices=["host", "device"], default="host",
                    help="device: the cluster file is parsed on the GPU (parse_clusters_device) and temp_dir/edge_list_csr.npz is written")
    ap.add_argument("--no-edge-list-npy", action="store_true",
                    help="--parse device: do not write edge_list.npy as well (building its object array costs what the device parse saves)")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    res, chrom_list, temp_dir = config["resolution"], config["chrom_list"], config["temp_dir"]
    bin2node, _, node2chrom, chrom_range = build_node_dict(config["chrom_size"], chrom_list, res, temp_dir)
    device_parse = args.parse == "device"
    if device_parse:
        clusters = parse_clusters_device(config["cluster_path"], chrom_list, chrom_range, res, config["max_cluster_size"])
        save_clusters_csr(temp_dir, clusters, edge_list_npy=not args.no_edge_list_npy)
        n_clusters = len(clusters[1]) - 1
    else:
        clusters = parse_clusters(config["cluster_path"], bin2node, chrom_list, res, config["max_cluster_size"], temp_dir)
        n_clusters = len(clusters)
    print("%d nodes, %d clusters" % (int(chrom_range.max()) - 1, n_clusters))
    N = int(chrom_range.max()) - 1
    if args.adj_from == "clusters":
        bound = config["max_cluster_size"] if args.adj_max_cluster_size is None else args.adj_max_cluster_size
        if bound > MAX_ADJ_CLUSTER:
            raise SystemExit("--adj-max-cluster-size is at most %d" % MAX_ADJ_CLUSTER)
        ca = ClusterAdj(N, node2chrom)
        step = 1 << 20                                                          # clusters per update
        if device_parse:
            adj_clusters = clusters if bound == config["max_cluster_size"] else parse_clusters_device(config["cluster_path"], chrom_list, chrom_range,
                                                                                                      res, bound)
            ids_d, off = adj_clusters[0], adj_clusters[1].cpu().numpy()
            n_adj = len(off) - 1
            for s in range(0, n_adj, step):                                     # slices of the device CSR: the ids stay on the device
                o = off[s:s + step + 1]
                ca.update((ids_d[int(o[0]):int(o[-1])], o - o[0]), args.adj_weight)
        else:
            adj_clusters = clusters if bound == config["max_cluster_size"] else parse_clusters(config["cluster_path"], bin2node, chrom_list, res, bound)
            n_adj = len(adj_clusters)
            for s in range(0, n_adj, step):
                ca.update(adj_clusters[s:s + step], args.adj_weight)
        intra, inter = ca.finish()
        if ca.status()[0] & _lib.STATUS_BAD_ID:
            raise IndexError("a cluster with ids that are not ascending or outside 1 .. %d was left out" % N)
        print("%d clusters, %d pairs -> intra_adj.npy / inter_adj.npy" % (n_adj, ca.n_pairs))
        save_adj(temp_dir, intra, inter)
        return
    try:
        import h5py
    except ImportError:
        raise SystemExit("h5py is not installed: load the cooler's bins / pixels yourself and call process.pixels_to_adj, or build the "
                         "adjacency from the cluster file with --adj-from clusters")
    f = h5py.File(config["mcool_path"], "r")["resolutions"][str(res)]
    i2n = cool_index2node(np.array(f["bins"]["chrom"]), np.array(f["bins"]["start"]), np.array(f["chroms"]["name"]).astype("str"),
                          chrom_list, bin2node)
    weights = f["pixels"]["balanced"] if "balanced" in f["pixels"].keys() else f["pixels"]["count"]       # process.py:147-150
    out, step = None, 1 << 24
    for s in range(0, len(weights), step):
        out = pixels_to_adj(f["pixels"]["bin1_id"][s:s + step], f["pixels"]["bin2_id"][s:s + step], weights[s:s + step], i2n, node2chrom, N, out=out)
    save_adj(temp_dir, *out)


if __name__ == "__main__":
    main()
