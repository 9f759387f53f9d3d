"""The cluster file parsed on the device (matcha_amd/process.py's parse_clusters_device, csrc/cluster_text.hip).  Integer work:
every comparison is EQUALITY of ids and offsets with the host parser ``parse_clusters``, which tests/test_process_features.py and
tests/test_cpu_cluster_text.py pin to the reference's own parse_file (g9_process.npz, cluster_text_edge.npz)."""
import builtins
import json

import numpy as np
import pytest
import torch

from matcha_amd import _lib
from matcha_amd import kmers as KM
from matcha_amd import process as PC
from tests import cluster_text_ref as R
from tests.helpers import gold

pytestmark = pytest.mark.gpu
KERNELS = ("cluster_text_count_kernel", "cluster_text_count_sum_kernel", "cluster_text_init_kernel", "cluster_text_span_kernel",
           "cluster_text_verify_kernel", "cluster_text_scatter_kernel", "cluster_text_lines_kernel", "cluster_text_items_kernel",
           "cluster_text_flag_kernel", "cluster_text_linecount_kernel", "cluster_text_emit_kernel", "cluster_text_offsets_kernel")


@pytest.fixture(scope="module")
def fx():
    return R.edge_fixture()


@pytest.fixture(scope="module")
def g9():
    g = gold("g9_process.npz")
    return g, R.Genome(g["sizes_text"], ["chr1", "chr2", "chrX"], 1000000)


def device(genome, text, max_cluster_size, **kw):
    ids, offsets = PC.parse_clusters_device(text, genome.chrom_list, genome.chrom_range, genome.res, max_cluster_size, **kw)
    assert ids.is_cuda and offsets.is_cuda and ids.dtype == torch.int32 and offsets.dtype == torch.int64 and ids.dim() == offsets.dim() == 1
    return ids.cpu().numpy(), offsets.cpu().numpy()


def same(got, want):
    return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def test_g9_cluster_file_at_every_chunking(g9, tmp_path):
    g, genome = g9
    text = str(g["cluster_text"]).encode()
    max_size = int(g["max_cluster_size"])
    want = (g["edge_flat"].astype(np.int32), np.concatenate([[0], np.cumsum(g["edge_len"])]).astype(np.int64))
    with _lib.launch_log() as log:
        whole = device(genome, text, max_size)
    assert same(whole, want) and len(want[1]) > 100
    assert all(log.counts.get(k, 0) == 1 for k in KERNELS), log.counts       # one chunk: every kernel of the parser once
    longest = max(len(l) for l in text.split(b"\n")) + 1
    small = longest + 1                                                       # just above the longest line (the skipped one of 301 items)
    assert len(list(PC._text_chunks(text, small))) >= 5
    with _lib.launch_log() as log:
        cut = device(genome, text, max_size, chunk_bytes=small)
    assert same(cut, want) and log.counts["cluster_text_items_kernel"] >= 5
    for size in (small + 7, 3 * small, len(text) - 1, len(text)):
        assert same(device(genome, text, max_size, chunk_bytes=size), want), size
    path = tmp_path / "x.cluster"                                             # and from the file
    path.write_bytes(text)
    assert same(device(genome, str(path), max_size, chunk_bytes=small), want) and same(device(genome, str(path), max_size), want)


def test_edge_fixture_accepted_cases_bit_for_bit(fx):
    g, genome = fx
    for name in (str(n) for n in g["accepted"]):
        text, max_size = g["text_" + name].tobytes(), int(g["max_" + name])
        want = R.fixture_csr(g, name)
        assert same(device(genome, text, max_size), want), name
        if len(text) > 40:                                                    # and cut into chunks of whole lines
            small = max(len(l) for l in text.replace(b"\r", b"\n").split(b"\n")) + 2
            assert same(device(genome, text, max_size, chunk_bytes=small), want), name


def test_edge_fixture_errors_keep_the_class_and_name_the_offset(fx):
    g, genome = fx
    for name in (str(n) for n in g["errors"]):
        text, max_size, off = g["text_" + name].tobytes(), int(g["max_" + name]), int(g["off_" + name])
        cls = getattr(builtins, str(g["exc_" + name]))
        with pytest.raises(cls, match="byte offset %d:" % off) as e:
            device(genome, text, max_size)
        assert type(e.value) is cls, name
        pad = b"c\tchr1:5\tchr1:1500000\n" * 7                                # behind other chunks: the offset is the file's
        small = max(max(len(l) for l in text.replace(b"\r", b"\n").split(b"\n")) + 2, len(pad) // 7)
        with pytest.raises(cls, match="byte offset %d:" % (len(pad) + off)):
            device(genome, pad + text, max_size, chunk_bytes=small)


@pytest.mark.parametrize("item", [b"chr1:+5", b"chr1: 5", b"chr1:2_500", b"chr1:-5", b"chr1:5 ", b"chr1:\xc2\xa05", b"chr\xc3\xa9:5", b"chr1:x", b"chr1:"])
def test_narrower_grammar_is_a_value_error(fx, item):
    _, genome = fx
    front = b"c\tchr1:5\tchr1:1500000\nc\tchr10:0\t"
    text = front + item + b"\tchr1:1500000\n"
    # the item's own offset; a non-ASCII byte in an unlisted NAME is the one thing wrong with its item, and is named itself
    off = len(front) + (item.index(b"\xc3") if b"\xc3" in item else 0)
    with pytest.raises(ValueError, match="byte offset %d:" % off) as e:
        device(genome, text, 6)
    assert type(e.value) is ValueError
    # 19 digits lie past every chromosome, whatever they spell; 17 zeros and a digit are a position
    with pytest.raises(KeyError, match="byte offset %d:" % len(front)):
        device(genome, front + b"chr1:" + b"0" * 18 + b"5\n", 6)
    short = front + b"chr1:" + b"0" * 17 + b"5\n"
    assert same(device(genome, short, 6), genome.host(short, 6))
    # a non-ASCII byte is refused wherever it stands, a skipped line included
    with pytest.raises(ValueError, match="byte offset 2: byte 0xc3"):
        device(genome, b"id\xc3\xa9\tchr1:5\n" + text[:len(front)], 6)


def test_malformed_items_on_a_skipped_line_raise_nothing(fx):
    _, genome = fx
    good = b"c\tchr1:5\tchr1:1500000\n"
    text = b"one\tchr1:+5\n" + good + b"\t".join([b"many"] + [b"chr1:+5", b"::", b"", b"chr1:99999999999999999999", b"chr1"] * 21) + b"\n" + good
    want = genome.host(text, 2)
    assert want[1].tolist() == [0, 2, 4] and same(device(genome, text, 2), want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_against_the_host_parser(fx, seed):
    _, genome = fx
    text = R.fuzz_text(genome, seed)
    assert 100_000 < len(text) < 500_000 and b"\r\n" in text and b"\n\n" in text
    want = genome.host(text, 6)
    assert len(want[1]) > 100
    assert same(device(genome, text, 6), want)
    assert same(device(genome, text, 6, chunk_bytes=4096), want)
    assert same(device(genome, text, 25), genome.host(text, 25))


def test_one_line_of_40000_items(fx):
    """50 max = 50 000: a kept line of 40 000 items (far longer than a workgroup's span, more than 2^15 items), a skipped one of 50 001 and 500
    two-item lines around them.  The genome is one chromosome of 1 200 bins, so the long line collapses to at most 1 000 nodes... or is dropped."""
    rng = np.random.default_rng(4)
    genome = R.Genome("chrL\t%d\n" % (1199 * 1000), ["chrL"], 1000)
    assert genome.n_nodes == 1200
    two = lambda: b"t\tchrL:%d\tchrL:%d\n" % tuple(rng.integers(0, 1199000, size=2))
    kept = b"\t".join([b"kept"] + [b"chrL:%d" % p for p in rng.integers(0, 990 * 1000, size=40000)]) + b"\n"          # <= 990 bins
    dropped = b"\t".join([b"wide"] + [b"chrL:%d" % p for p in rng.integers(0, 1199000, size=40000)]) + b"\n"        # ~1 200 bins: over 1 000
    skipped = b"\t".join([b"skipped"] + [b"chrL:5", b"chrL:1500"] * 25000 + [b"chrL:x"]) + b"\n"                     # 50 001 items, one malformed
    text = b"".join(two() for _ in range(250)) + kept + skipped + dropped + b"".join(two() for _ in range(250))
    want = genome.host(text, 1000)
    sizes = np.diff(want[1])
    assert 900 < sizes.max() <= 1000 and (sizes > 2).sum() == 1 and len(sizes) > 400
    got = device(genome, text, 1000)
    assert same(got, want)
    assert same(device(genome, text, 1000, chunk_bytes=max(len(kept), len(skipped), len(dropped)) + 1), want)


def test_empty_results(fx):
    _, genome = fx
    empty = (np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64))
    skipped_only = b"a\tchr1:5\nb\n\n" + b"\t".join([b"c"] + [b"chr1:5"] * 301) + b"\nd\tchr1:5\tchr1:6\ne\tchrY:5\tchrY:9000000\n"
    for text in (b"", b"\n", b"x", b"\r\n\r\n", b"id\tchr1:5", skipped_only, skipped_only[:-1]):
        assert same(device(genome, text, 6), empty), text[:20]
    assert same(device(genome, b"c\tchr1:5\tchr1:1500000", 6), (np.asarray([1, 2], dtype=np.int32), np.asarray([0, 2], dtype=np.int64)))      # no terminator


def test_consumers_take_the_device_csr(g9):
    g, genome = g9
    text = str(g["cluster_text"]).encode()
    ids_d, off_d = PC.parse_clusters_device(text, genome.chrom_list, genome.chrom_range, genome.res, 11)
    ids, off = ids_d.cpu().numpy(), off_d.cpu().numpy()
    lists = [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    N = genome.n_nodes
    n2c = PC.node2chrom_array(genome.node2chrom, N)
    a = PC.ClusterAdj(N, n2c).update((ids_d, off_d), "two_over_n")
    b = PC.ClusterAdj(N, n2c).update(lists, "two_over_n")
    assert torch.equal(a._acc, b._acc) and a._acc.dtype == torch.int64 and a._acc.any() and a.n_pairs == b.n_pairs and a.status() == [0, 0, 0, 0]
    for x, y in zip(a.finish(), b.finish()):
        assert x.dtype == torch.float64 and torch.equal(x, y)
    for x, y in zip(PC.clusters_to_adj((ids_d, off_d), n2c, N), PC.clusters_to_adj(lists, n2c, N)):
        assert torch.equal(x, y)
    half = len(off) // 2                                                      # a slice of the device ids, offsets as numpy
    c = PC.ClusterAdj(N, n2c).update((ids_d[:off[half]], off[:half + 1]), "two_over_n").update((ids_d[off[half]:], off_d[half:] - off_d[half]), "two_over_n")
    assert torch.equal(a._acc, c._acc)
    for k in (2, 3):
        for cap in (0, 200):
            rows_d, freq_d = KM.generate_kmers((ids_d, off_d), k, 0, 11, 1, N + 1, max_combos_per_launch=cap)
            rows_l, freq_l = KM.generate_kmers(lists, k, 0, 11, 1, N + 1, max_combos_per_launch=cap)
            assert len(rows_l) > 50 and np.array_equal(rows_d, rows_l) and np.array_equal(freq_d, freq_l), (k, cap)
    rows_d, freq_d = KM.generate_kmers((ids_d, off_d), 2, 1, 11, 2)         # n_nodes from the device ids
    rows_l, freq_l = KM.generate_kmers(lists, 2, 1, 11, 2)
    assert np.array_equal(rows_d, rows_l) and np.array_equal(freq_d, freq_l) and len(rows_l)
    with pytest.raises(ValueError, match="offsets"):
        PC.ClusterAdj(N, n2c).update((ids_d, off_d[:-1]))


def test_end_to_end_drivers(g9, tmp_path):
    g, _ = g9
    sizes, clusters = tmp_path / "sizes.txt", tmp_path / "x.cluster"
    sizes.write_text(str(g["sizes_text"]))
    clusters.write_text(str(g["cluster_text"]))
    out = {}
    for mode in ("host", "device"):
        temp = tmp_path / mode
        cfg = {"resolution": 1000000, "chrom_list": ["chr1", "chr2", "chrX"], "temp_dir": str(temp), "chrom_size": str(sizes),
               "cluster_path": str(clusters), "max_cluster_size": 6, "k-mer_size": [2, 3], "min_distance": 0, "min_freq_cutoff": 1}
        config = tmp_path / (mode + ".JSON")
        config.write_text(json.dumps(cfg))
        PC.main(["--config", str(config), "--adj-from", "clusters", "--adj-max-cluster-size", "9", "--parse", mode])
        KM.main(["--config", str(config)] + (["--clusters", "csr"] if mode == "device" else []))
        out[mode] = {n: np.load(temp / n, allow_pickle=True) for n in ("intra_adj.npy", "inter_adj.npy", "edge_list.npy", "all_2_counter.npy",
                                                                          "all_2_freq_counter.npy", "all_3_counter.npy", "all_3_freq_counter.npy")}
    for name, want in out["host"].items():
        got = out["device"][name]
        if name == "edge_list.npy":
            assert [list(e) for e in got] == [list(e) for e in want] and len(want) == len(g["edge_len"])
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want) and want.any(), name
    with np.load(tmp_path / "device" / "edge_list_csr.npz") as z:
        assert np.array_equal(z["ids"], g["edge_flat"]) and z["ids"].dtype == np.int32
        assert np.array_equal(z["offsets"], np.concatenate([[0], np.cumsum(g["edge_len"])])) and z["offsets"].dtype == np.int64
    assert not (tmp_path / "host" / "edge_list_csr.npz").exists()
    temp = tmp_path / "device"                                               # --no-edge-list-npy: the CSR alone
    (temp / "edge_list.npy").unlink()
    PC.main(["--config", str(tmp_path / "device.JSON"), "--adj-from", "clusters", "--parse", "device", "--no-edge-list-npy"])
    assert not (temp / "edge_list.npy").exists() and (temp / "edge_list_csr.npz").exists()
