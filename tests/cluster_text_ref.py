"""What tests/test_cpu_cluster_text.py and tests/test_hip_cluster_text.py share: the genome of tests/golden/cluster_text_edge.npz, the host parser
``process.parse_clusters`` as the checker of a text (it is pinned to the reference by g9_process.npz and by the edge fixture), and the random
cluster files of the fuzz test."""
import os
import tempfile

import numpy as np

from matcha_amd import process as PC
from tests.helpers import gold

STRIP = [b" ", b"\t", b"\x0b", b"\x0c", b"\x1c", b"\x1d", b"\x1e", b"\x1f"]      # str.strip()'s set without the two line terminators


class Genome:
    """chrom_list, res, and the node dictionaries ``build_node_dict`` makes from a size file's text."""

    def __init__(self, sizes_text, chrom_list, res):
        self.chrom_list, self.res = [str(c) for c in chrom_list], int(res)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "sizes.txt")
            with open(path, "w") as f:
                f.write(str(sizes_text))
            self.bin2node, _, self.node2chrom, self.chrom_range = PC.build_node_dict(path, self.chrom_list, self.res)
        self.n_nodes = int(self.chrom_range.max()) - 1

    def host(self, text: bytes, max_cluster_size: int):
        """parse_clusters on ``text`` -> (ids int32, offsets int64); its exceptions pass through."""
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "x.cluster")
            with open(path, "wb") as f:
                f.write(text)
            clusters = PC.parse_clusters(path, self.bin2node, self.chrom_list, self.res, int(max_cluster_size))
        return csr(clusters)


def csr(clusters):
    offsets = np.zeros(len(clusters) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clusters], out=offsets[1:])
    ids = np.asarray([v for c in clusters for v in c], dtype=np.int32)
    return ids, offsets


def edge_fixture():
    g = gold("cluster_text_edge.npz")
    return g, Genome(g["sizes_text"], g["chrom_list"], g["res"])


def fixture_csr(g, name):
    offsets = np.concatenate([[0], np.cumsum(g["len_" + name])]).astype(np.int64)
    return g["flat_" + name].astype(np.int32), offsets


def fuzz_text(genome: Genome, seed: int, n_lines: int = 2000) -> bytes:
    """About 100 bytes per line: 0 .. 40 items; listed names that are prefixes of each other, unlisted names; positions on the first and the
    last bin and in between; duplicates; the three terminators mixed; blanks of the strip set at both ends; empty lines."""
    rng = np.random.default_rng(seed)
    sizes = {c: int(hi - lo) * genome.res for c, (lo, hi) in zip(genome.chrom_list, genome.chrom_range)}      # positions below this have a bin
    names = genome.chrom_list + ["chrY", "chr1_rando", "chr100", "chr"]
    out = []
    for k in range(n_lines):
        kind = rng.random()
        n = 0 if kind < 0.08 else int(rng.integers(0, 41)) if kind < 0.5 else int(rng.integers(1, 9))
        items = []
        for _ in range(n):
            name = names[int(rng.integers(0, len(names)))]
            top = sizes.get(name, 5 * genome.res)
            r = rng.random()
            pos = 0 if r < 0.1 else top - 1 if r < 0.2 else top - genome.res if r < 0.25 else int(rng.integers(0, top))
            items.append(b"%s:%d" % (name.encode(), pos))
            if rng.random() < 0.15:
                items.append(items[int(rng.integers(0, len(items)))])
        lead = b"".join(STRIP[int(i)] for i in rng.integers(0, len(STRIP), size=int(rng.integers(0, 4)))) if rng.random() < 0.3 else b""
        trail = b"".join(STRIP[int(i)] for i in rng.integers(0, len(STRIP), size=int(rng.integers(0, 4)))) if rng.random() < 0.3 else b""
        body = b"" if kind < 0.04 else b"\t".join([b"id%d" % k] + items)
        out.append(lead + body + trail + [b"\n", b"\r\n", b"\r"][int(rng.integers(0, 3))])
    text = b"".join(out)
    return text[:-1] if seed % 2 and text.endswith(b"\n") and not text.endswith(b"\r\n") else text
