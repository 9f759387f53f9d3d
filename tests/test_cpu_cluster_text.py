"""The cluster file parsed on the device (matcha_amd/process.py's parse_clusters_device, csrc/cluster_text.hip), without a GPU:
the host parser -- the checker of the GPU tests -- against the reference's own parse_file on every edge case of the contract
(tests/golden/cluster_text_edge.npz, written by tools/make_cluster_text_golden.py from the reference's source), the ABI surface, the workspace
queries and every refusal that comes before a device call, the chunk cutting, and the stand-alone host driver
tests/host/cluster_parse_checks under ASan + UBSan."""
import builtins
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from matcha_amd import _lib
from matcha_amd import kmers as KM
from matcha_amd import process as PC
from tests import cluster_text_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["matcha_cluster_text_count_workspace_bytes", "matcha_cluster_text_count", "matcha_cluster_text_workspace_bytes", "matcha_cluster_text_parse"]
KERNELS = ["cluster_text_count_kernel", "cluster_text_span_kernel", "cluster_text_scatter_kernel", "cluster_text_lines_kernel",
           "cluster_text_items_kernel", "cluster_text_flag_kernel", "cluster_text_linecount_kernel", "cluster_text_emit_kernel",
           "cluster_text_offsets_kernel"]


@pytest.fixture(scope="module")
def fx():
    return R.edge_fixture()


# ---- the checker on the adversarial cases ------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases_the_contract_names(fx):
    g, genome = fx
    assert genome.chrom_list == ["chr1", "chr10", "chr1_random", "chrX"] and genome.res == 1000000
    assert np.array_equal(genome.chrom_range, g["chrom_range"]) and genome.chrom_range.tolist() == [[1, 15], [15, 24], [24, 28], [28, 35]]
    assert len(g["accepted"]) >= 19 and len(g["errors"]) >= 16
    assert {str(g["exc_" + str(n)]) for n in g["errors"]} == {"EOFError", "KeyError", "ValueError"}
    text = lambda n: g["text_" + n].tobytes()
    assert b"\r\n" in text("newlines") and b"\r" in text("newlines").replace(b"\r\n", b"") and not text("newlines").endswith((b"\n", b"\r"))
    assert text("leading_tabs").startswith(b"\tchr1:5\t") and g["len_leading_tabs"].tolist() == [2, 2]
    assert all(bytes([b]) in text("strip_set") for b in (0x0b, 0x0c, 0x1c, 0x1d, 0x1e, 0x1f, 0x20))
    assert text("prefilter_over").split(b"\n")[0].count(b"\t") == 101 and g["len_prefilter_over"].tolist() == [2]
    assert text("prefilter_exact").split(b"\n")[0].count(b"\t") == 100 and g["len_prefilter_exact"].tolist() == [2, 2]
    assert g["flat_name_prefixes"].tolist()[:4] == [1, 15, 24, 28]
    assert g["flat_last_bins"].tolist() == [13, 14, 23, 27, 28, 34]
    assert sum(g["text_" + str(n)].size for n in list(g["accepted"]) + list(g["errors"])) < 100_000
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cluster_text_edge.npz")) < 100_000
    assert all(g[k].dtype.kind in "iuU" for k in g.files)                     # text, bounds, results and names: no program text


def test_host_parser_equals_the_reference_on_every_accepted_case(fx):
    g, genome = fx
    for name in (str(n) for n in g["accepted"]):
        ids, offsets = genome.host(g["text_" + name].tobytes(), int(g["max_" + name]))
        want_ids, want_off = R.fixture_csr(g, name)
        assert np.array_equal(ids, want_ids) and np.array_equal(offsets, want_off), name


def test_host_parser_raises_the_reference_s_exception_classes(fx):
    g, genome = fx
    for name in (str(n) for n in g["errors"]):
        cls = getattr(builtins, str(g["exc_" + name]))
        text = g["text_" + name].tobytes()
        with pytest.raises(cls):
            genome.host(text, int(g["max_" + name]))
        off = int(g["off_" + name])
        assert text[off - 1:off] == b"\t" and 0 < off <= len(text), name       # the offending item starts behind a tab


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_signatures():
    lib = _lib.load()
    assert lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "matcha_hip.h")) as f:
        header = f.read()
    assert "#define MATCHA_ABI_VERSION 7" in header
    for name in NEW:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    S = _lib.SIGNATURES
    assert S["matcha_cluster_text_count_workspace_bytes"][0] is C.c_size_t and len(S["matcha_cluster_text_count_workspace_bytes"][1]) == 1
    assert S["matcha_cluster_text_count"][0] is C.c_int and len(S["matcha_cluster_text_count"][1]) == 6
    assert S["matcha_cluster_text_workspace_bytes"][0] is C.c_size_t and len(S["matcha_cluster_text_workspace_bytes"][1]) == 3
    assert S["matcha_cluster_text_parse"][0] is C.c_int and len(S["matcha_cluster_text_parse"][1]) == 21
    for word, value in (("NAME_MAX", _lib.CLUSTER_TEXT_NAME_MAX), ("CHROM_MAX", _lib.CLUSTER_TEXT_CHROM_MAX), ("ESPLIT", _lib.CLUSTER_TEXT_ESPLIT),
                        ("EBIN", _lib.CLUSTER_TEXT_EBIN), ("EGRAMMAR", _lib.CLUSTER_TEXT_EGRAMMAR), ("ENONASCII", _lib.CLUSTER_TEXT_ENONASCII),
                        ("ECOUNT", _lib.CLUSTER_TEXT_ECOUNT)):
        assert "#define MATCHA_CLUSTER_TEXT_%s %d" % (word, value) in header
    for phrase in ("1 .. 18 ASCII digits", "19 or more digits", "byte >= 0x80", "2_500"):      # the narrower grammar is documented where the ABI is
        assert phrase in header
    with open(os.path.join(ROOT, "matcha_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    for kernel in KERNELS:
        assert "ZERO_SCRATCH += " + kernel in mk                              # the build's scratch gate covers the new kernels


def test_workspace_queries():
    lib = _lib.load()
    W, CW = lib.matcha_cluster_text_workspace_bytes, lib.matcha_cluster_text_count_workspace_bytes
    assert CW(0) == CW((1 << 31) - 1) == 8192 and CW(-1) == 0 and CW(1 << 31) == 0
    assert W(-1, 1, 0) == 0 and W(1 << 31, 1, 0) == 0 and W(10, 0, 0) == 0 and W(10, 12, 0) == 0 and W(10, 1, 11) == 0 and W(10, 6, 6) == 0
    sizes = [W(n, nl, nt) for n, nl, nt in ((0, 1, 0), (100, 1, 0), (100, 5, 12), (1 << 20, 1, 0), (1 << 20, 1 << 15, 0), (1 << 20, 1 << 15, 1 << 18))]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[5] - sizes[4] >= (1 << 18) * 24 and sizes[4] - sizes[3] >= (1 << 15) * 24 - 5 * 256 and sizes[3] >= (1 << 16) * 8
    assert W((1 << 28), 1 << 22, 1 << 25) < 3 << 30                           # a 256 MiB chunk of SPRITE-like text: under 3 GiB


def _table(names=("chr1", "chr10"), first=(1, 15), bins=(14, 9)):
    t = np.zeros((len(names), 32), dtype=np.uint8)
    for i, n in enumerate(names):
        raw = n if isinstance(n, bytes) else n.encode()
        t[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return t, np.asarray(first, dtype=np.int32), np.asarray(bins, dtype=np.int32)


def test_abi_refusals_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 128)()
    base = (C.addressof(host) + 255) // 256 * 256                             # stands for device memory: never dereferenced
    p = C.c_void_p(base)
    err = lambda: lib.matcha_last_error().decode()
    t, f, b = _table()
    tp, fp, bp = (a.ctypes.data_as(C.c_void_p) for a in (t, f, b))
    need = lib.matcha_cluster_text_workspace_bytes(100, 5, 12)
    cneed = lib.matcha_cluster_text_count_workspace_bytes(100)

    def parse(text=p, n=100, nl=5, nt=12, names=tp, first=fp, bins=bp, n_chrom=2, res=1000, max_size=6, n_nodes=23, ids=p, ids_cap=12, offsets=p,
              offsets_cap=6, n_clusters=p, n_ids=p, status=p, ws=p, ws_bytes=need):
        return lib.matcha_cluster_text_parse(text, n, nl, nt, names, first, bins, n_chrom, res, max_size, n_nodes, ids, ids_cap, offsets, offsets_cap,
                                             n_clusters, n_ids, status, ws, ws_bytes, None)
    with _lib.launch_log() as log:
        K = lib.matcha_cluster_text_count
        assert K(p, -1, p, p, cneed, None) == -22 and "n=-1" in err()
        assert K(p, 1 << 31, p, p, cneed, None) == -22 and "n=" in err()
        assert K(p, 100, None, p, cneed, None) == -22 and "null pointer" in err()
        assert K(None, 100, p, p, cneed, None) == -22 and "null text" in err()
        assert K(C.c_void_p(base + 8), 100, p, p, cneed, None) == -22 and "aligned" in err()
        assert K(p, 100, p, p, cneed - 1, None) == -22 and "too small" in err()
        assert parse(n=-1) == -22 and "n=-1" in err()
        assert parse(nl=0) == -22 and "cannot be the counts" in err()
        assert parse(nt=101) == -22 and "cannot be the counts" in err()
        assert parse(nl=60, nt=60) == -22 and "cannot be the counts" in err()
        assert parse(n_chrom=0) == -22 and "n_chrom=0" in err()
        assert parse(n_chrom=257) == -22 and "n_chrom=257" in err()
        assert parse(res=0) == -22 and "res=0" in err()
        assert parse(res=1 << 31) == -22 and "res=" in err()
        assert parse(max_size=0) == -22 and "max_cluster_size=0" in err()
        assert parse(n_nodes=0) == -22 and "n_nodes=0" in err()
        for name in ("names", "first", "bins", "ids", "offsets", "n_clusters", "n_ids", "status", "ws"):
            assert parse(**{name: None}) == -22 and "null pointer" in err(), name
        assert parse(text=None) == -22 and "null text" in err()
        assert parse(text=C.c_void_p(base + 4)) == -22 and "aligned" in err()
        assert parse(ws=C.c_void_p(base + 64)) == -22 and "aligned" in err()
        assert parse(ids_cap=11) == -22 and "ids_cap=11" in err()
        assert parse(offsets_cap=5) == -22 and "offsets_cap=5" in err()
        assert parse(ws_bytes=need - 1) == -22 and "too small" in err()
        # the table
        for names, first, bins, word in ((("chr1", "chr1"), (1, 15), (14, 9), "duplicate name"), (("chr1", ""), (1, 15), (14, 9), "empty name"),
                                         (("chr1", "chr 2"), (1, 15), (14, 9), "chromosome 1: name"), (("chr1", "chr\t2"), (1, 15), (14, 9), "name"),
                                         (("chr1", "chr:2"), (1, 15), (14, 9), "name"), (("chr1", b"chr\xc3\xa9"), (1, 15), (14, 9), "name"),
                                         (("chr1", "chr10"), (0, 15), (14, 9), "chromosome 0: node range"),
                                         (("chr1", "chr10"), (1, 15), (14, 10), "chromosome 1: node range"),
                                         (("chr1", "chr10"), (1, 15), (14, 0), "node range")):
            t2, f2, b2 = _table(names, first, bins)
            assert parse(names=t2.ctypes.data_as(C.c_void_p), first=f2.ctypes.data_as(C.c_void_p), bins=b2.ctypes.data_as(C.c_void_p)) == -22
            assert word in err(), (names, err())
        t2, f2, b2 = _table(("chr1",), (1,), (1 << 23,))
        assert parse(names=t2.ctypes.data_as(C.c_void_p), first=f2.ctypes.data_as(C.c_void_p), bins=b2.ctypes.data_as(C.c_void_p), n_chrom=1,
                     res=(1 << 31) - 1, n_nodes=1 << 24) == -22 and "2^53" in err()
    assert not log.counts


# ---- the host side of parse_clusters_device ----------------------------------------------------------------------------------------------
def test_chrom_table_refusals_come_before_the_device():
    cr = [[1, 15], [15, 24]]
    dev = dict(device="cpu")
    text = b"c\tchr1:5\tchr1:1500000\n"
    for names, word in ((["chr1", "chr1"], "twice"), (["chr1", ""], "empty"), (["chr1", "chré"], "not ASCII"), (["chr1", "chr\t2"], "tab"),
                        (["chr1", "chr:2"], "colon"), (["chr1", "chr 2"], "blank"), (["chr1", "chr\x1c"], "control"), (["chr1", "c" * 33], "longer than 32"),
                        (["chr1", 7], "not a string")):
        with pytest.raises(ValueError, match=word):
            PC.parse_clusters_device(text, names, cr, 1000000, 6, **dev)
    many = ["c%d" % i for i in range(257)]
    with pytest.raises(ValueError, match="256"):
        PC.parse_clusters_device(text, many, [[i + 1, i + 2] for i in range(257)], 1000000, 6, **dev)
    with pytest.raises(ValueError, match="2 chromosome names for 1 rows"):
        PC.parse_clusters_device(text, ["chr1", "chr10"], [[1, 15]], 1000000, 6, **dev)
    for res in (0, -5, 1 << 31, 2.5):
        with pytest.raises(ValueError, match="res"):
            PC.parse_clusters_device(text, ["chr1", "chr10"], cr, res, 6, **dev)
    with pytest.raises(ValueError, match="2\\^53"):
        PC.parse_clusters_device(text, ["chr1"], [[1, 1 + (1 << 23)]], (1 << 31) - 1, 6, **dev)
    with pytest.raises(ValueError, match="start < end"):
        PC.parse_clusters_device(text, ["chr1", "chr10"], [[1, 15], [15, 15]], 1000000, 6, **dev)
    with pytest.raises(ValueError, match="max_cluster_size"):
        PC.parse_clusters_device(text, ["chr1", "chr10"], cr, 1000000, 0, **dev)
    names, first, bins, n_nodes = PC.cluster_chrom_table(["chr1", "c" * 32], cr, 1000000)
    assert names.shape == (2, 32) and names[0].tobytes() == b"chr1" + b"\0" * 28 and names[1].tobytes() == b"c" * 32
    assert first.tolist() == [1, 15] and bins.tolist() == [14, 9] and n_nodes == 23 and first.dtype == np.int32
    # accepted by the host checks: now it needs the device -- also for an empty file
    for src in (text, b""):
        with pytest.raises(_lib.MatchaHipError, match="no CPU fallback"):
            PC.parse_clusters_device(src, ["chr1", "chr10"], cr, 1000000, 6, **dev)


def test_a_line_longer_than_chunk_bytes_is_refused_with_its_offset(tmp_path):
    cr, names = [[1, 15], [15, 24]], ["chr1", "chr10"]
    short = b"c\tchr1:5\tchr1:1500000\n"
    long = b"c\t" + b"\t".join([b"chr1:5"] * 40) + b"\n"
    with pytest.raises(ValueError, match="byte offset 0 is longer than chunk_bytes = 64"):
        PC.parse_clusters_device(long + short, names, cr, 1000000, 6, chunk_bytes=64, device="cpu")
    path = tmp_path / "x.cluster"
    path.write_bytes(short * 5 + long + short)
    chunks = PC._text_chunks(str(path), 64)
    assert next(chunks)[2] == 2 * len(short)                                  # the first chunk is cut and handed out; the long line is met later
    with pytest.raises(ValueError, match="byte offset %d is longer" % (5 * len(short))):
        list(chunks)
    for bad in (0, 1 << 31):
        with pytest.raises(ValueError, match="chunk_bytes"):
            next(PC._text_chunks(short, bad))


def test_chunks_are_whole_lines_and_join_to_the_file(tmp_path):
    rng = np.random.default_rng(8)
    lines = [bytes(rng.integers(97, 123, size=int(rng.integers(0, 30))).astype(np.uint8)) + [b"\n", b"\r\n", b"\r"][int(rng.integers(0, 3))]
             for _ in range(400)]
    for tail in (b"", b"last line without a terminator"):
        text = b"".join(lines) + tail
        path = tmp_path / "t.txt"
        path.write_bytes(text)
        for src in (text, str(path), bytearray(text)):
            for size in (32, 33, 100, 4096, len(text) - 1, len(text), len(text) + 1, 1 << 28):
                got, at = [], 0
                for base, buf, length in PC._text_chunks(src, size):
                    piece = bytes(buf[:length])
                    assert base == at and 0 < length <= size
                    assert piece.endswith((b"\n", b"\r")) or at + length == len(text)
                    got.append(piece)
                    at += length
                assert b"".join(got) == text
    assert list(PC._text_chunks(b"", 64)) == []
    exact = b"x" * 63 + b"\n"                                                 # a buffer that ends with the file, with and without a terminator
    assert [c[2] for c in PC._text_chunks(exact, 64)] == [64] and [c[2] for c in PC._text_chunks(b"y" * 64, 64)] == [64]


def test_consumers_check_a_device_pair_s_offsets_on_the_host():
    """device_csr, which ClusterAdj.update and generate_kmers call for an (ids, offsets) pair with device ids, on CPU tensors: the ids are not
    touched, the offsets are checked as _clusters_csr checks a host pair; host pairs and lists go the way they went."""
    ids = torch.tensor([1, 2, 3, 4, 9], dtype=torch.int64)
    got, off = PC.device_csr((ids, torch.tensor([0, 3, 3, 5])), "cpu")
    assert got.dtype == torch.int32 and got.tolist() == [1, 2, 3, 4, 9] and off.dtype == np.int64 and off.tolist() == [0, 3, 3, 5]
    for bad in ([1, 3, 5], [0, 3, 4], [0, 4, 3, 5], []):
        with pytest.raises(ValueError, match="offsets"):
            PC.device_csr((ids, np.asarray(bad, dtype=np.int64)), "cpu")
    assert not PC._is_device_csr((ids, np.asarray([0, 5]))) and not PC._is_device_csr([[1, 2]]) and not PC._is_device_csr((ids.numpy(), np.asarray([0, 5])))
    ids_np, off_np = PC._clusters_csr((ids, np.asarray([0, 3, 3, 5])))        # a host pair: numpy, as before
    assert isinstance(ids_np, np.ndarray) and ids_np.dtype == np.int32 and off_np.tolist() == [0, 3, 3, 5]
    ids2, off2, lens = KM._csr([[1, 2, 3], [4, 9]])
    assert ids2.tolist() == [1, 2, 3, 4, 9] and off2.tolist() == [0, 3, 5] and lens.tolist() == [3, 2]


def test_save_clusters_csr_writes_both_files(tmp_path):
    ids, offsets = np.asarray([1, 3, 13, 1, 3], dtype=np.int32), np.asarray([0, 3, 5], dtype=np.int64)
    PC.save_clusters_csr(str(tmp_path), (torch.from_numpy(ids), torch.from_numpy(offsets)))
    with np.load(tmp_path / "edge_list_csr.npz") as z:
        assert z["ids"].dtype == np.int32 and z["offsets"].dtype == np.int64 and z["ids"].tolist() == ids.tolist() and z["offsets"].tolist() == [0, 3, 5]
    edge_list = np.load(tmp_path / "edge_list.npy", allow_pickle=True)
    assert edge_list.dtype == object and [list(e) for e in edge_list] == [[1, 3, 13], [1, 3]] and type(edge_list[0][0]) is int
    os.remove(tmp_path / "edge_list.npy")
    PC.save_clusters_csr(str(tmp_path), (ids, offsets), edge_list_npy=False)
    assert not os.path.exists(tmp_path / "edge_list.npy") and os.path.exists(tmp_path / "edge_list_csr.npz")


# ---- the host driver ---------------------------------------------------------------------------------------------------------------------
def test_host_driver_under_asan_ubsan():
    """tests/host/cluster_parse_checks, built by `make host-asan` with the other drivers and run stand-alone as tests/test_cpu_host_checks.py runs
    them: the workspace carving, every refusal of the two entries and of the chromosome table, MATCHA_EHIP from the first device call."""
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "cluster_parse_checks" in [w for line in f if line.startswith("HOST_DRIVERS") for w in line.split()]
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    run = subprocess.run([os.path.join(ROOT, "build", "host_asan", "cluster_parse_checks")], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert "ALL CLUSTER PARSE HOST CHECKS PASSED" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
