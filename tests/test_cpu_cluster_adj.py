"""Contact matrices from the clusters without a GPU (matcha_amd/process.py's ClusterAdj / clusters_to_adj, csrc/cluster_adj.hip's host side,
DESIGN.md 7.18): the numpy twin (tests/cluster_adj_ref.py) against the reference's own edgelist2adj / get_adjacency matrices
(tests/golden/cluster_adj_tiny.npz, written by tools/make_cluster_adj_golden.py from the reference's source), the ABI surface, the host-only
pair count, the refusals that come before any device call, ``process.main --adj-from clusters`` up to the device, and the stand-alone host
driver tests/host/cluster_adj_checks (pair unrank, argument checks) under ASan + UBSan."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from matcha_amd import _lib
from matcha_amd import process as PC
from tests import cluster_adj_ref as R
from tests.helpers import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["matcha_cluster_pairs_count", "matcha_cluster_adj_update", "matcha_cluster_adj_finish", "matcha_block_colmax_workspace_bytes",
       "matcha_block_colmax_normalise"]


@pytest.fixture(scope="module")
def g():
    return gold("cluster_adj_tiny.npz")


# ---- the fixture and the twin ------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_graph_the_tests_need(g):
    clusters = R.split_csr(g["ids"], g["offsets"])
    sizes = sorted(set(len(c) for c in clusters))
    assert int(g["n_nodes"]) == 70 and g["num"].tolist() == [30, 25, 15] and sizes == [2, 3, 5, 12, 40] and len(clusters) == 60
    assert all(R.cluster_ok(c, 70) for c in clusters)
    big = [c for c in clusters if len(c) == 40][0]
    assert set(g["node2chrom"][big].tolist()) == {0, 1, 2}
    assert sum(c == [4, 33] for c in clusters) == 7 and 70 not in set(g["ids"].tolist())
    assert g["weights"].min() >= 1 and g["weights"].max() <= 9 and (g["weights"] == np.rint(g["weights"])).all()
    assert g["adjacency_norm"].dtype == np.float32 and g["edgelist2adj"].dtype == np.float64
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cluster_adj_tiny.npz")) < 100_000


def test_twin_equals_the_reference_bit_for_bit(g):
    clusters = R.split_csr(g["ids"], g["offsets"])
    N = int(g["n_nodes"])
    one = R.adj_ref(clusters, N, "one")
    assert one.dtype == np.float64 and np.array_equal(one, g["edgelist2adj"])
    assert one[3, 32] == one[32, 3] and one[3, 32] >= 7 and not one[69].any() and not np.diag(one).any()
    w = R.adj_ref(clusters, N, g["weights"])
    assert np.array_equal(w.astype(np.float32).view(np.uint32), g["adjacency"].view(np.uint32))
    norm = R.block_colmax_ref(w, g["chrom_range"] - 1)
    assert np.array_equal(norm.astype(np.float32).view(np.uint32), g["adjacency_norm"].view(np.uint32))
    intra, inter = R.adj_ref(clusters, N, "one", g["node2chrom"])
    assert np.array_equal(intra + inter, one) and not (intra * inter).any() and inter.any() and intra.any()
    # a rejected cluster adds nothing; clusters without pairs are passed over
    acc, bad = R.acc_ref(clusters + [[5, 3, 9], [0, 4], [3, 71], [7], []], N)
    assert bad and np.array_equal(acc, R.acc_ref(clusters, N)[0])


def test_weights_in_fixed_point():
    lens = np.asarray([2, 3, 7, 1000])
    assert PC.cluster_weights_q(lens, "one").tolist() == [1 << 32] * 4
    q = PC.cluster_weights_q(lens, "two_over_n")
    assert q.dtype == np.int64 and q.tolist() == [1 << 32, int(np.rint(2.0 / 3.0 * 2.0 ** 32)), int(np.rint(2.0 / 7.0 * 2.0 ** 32)), 8589935]
    assert np.array_equal(q, R.weights_q(lens, "two_over_n"))
    assert PC.cluster_weights_q(lens, [0.5, -3.0, 2.0 ** -33, 2.0 ** 29]).tolist() == [1 << 31, -3 << 32, 0, 1 << 61]
    for bad in ([1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0, 1.0], [1.0, 2.0 ** 30, 1.0, 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError):
            PC.cluster_weights_q(lens, bad)
    with pytest.raises(ValueError):
        PC.cluster_weights_q(lens, "n_over_two")


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
    assert S["matcha_cluster_pairs_count"][0] is C.c_int64 and len(S["matcha_cluster_pairs_count"][1]) == 2
    assert S["matcha_cluster_adj_update"][0] is C.c_int and len(S["matcha_cluster_adj_update"][1]) == 9
    assert S["matcha_cluster_adj_finish"][0] is C.c_int and len(S["matcha_cluster_adj_finish"][1]) == 6
    assert S["matcha_block_colmax_workspace_bytes"][0] is C.c_size_t and len(S["matcha_block_colmax_workspace_bytes"][1]) == 2
    assert S["matcha_block_colmax_normalise"][0] is C.c_int and len(S["matcha_block_colmax_normalise"][1]) == 7
    with open(os.path.join(ROOT, "matcha_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    for kernel in ("cluster_pairs_update_kernel", "cluster_adj_finish_kernel", "block_colmax_normalise_kernel"):
        assert "ZERO_SCRATCH += " + kernel in mk                              # the build's scratch gate covers the new kernels


def test_pair_count():
    lib = _lib.load()

    def count(offsets):
        a = np.asarray(offsets, dtype=np.int64)
        return lib.matcha_cluster_pairs_count(a.ctypes.data_as(C.c_void_p), len(a) - 1)
    assert count([0]) == 0 and count([0, 2]) == 1 and count([0, 2, 5, 5, 6, 70, 1070]) == 1 + 3 + 0 + 0 + 2016 + 499500
    assert count([0, 65535]) == 65535 * 65534 // 2 and count([0, 65536]) == -1 and count([0, 3, 65539]) == -1
    assert count([0, 5, 3]) == -1
    assert lib.matcha_cluster_pairs_count(None, 1) == -1
    big = np.arange(0, 40000, dtype=np.int64) * 65535
    assert count(big) == 39999 * (65535 * 65534 // 2)


def test_abi_refusals_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    with _lib.launch_log() as log:
        U, F, Nm = lib.matcha_cluster_adj_update, lib.matcha_cluster_adj_finish, lib.matcha_block_colmax_normalise
        assert U(p, p, p, p, -1, 4, p, p, None) == -22 and "M=-1" in err()
        assert U(p, p, p, p, 1, 0, p, p, None) == -22 and "n_nodes=0" in err()
        assert U(p, p, p, p, 1, 4, None, p, None) == -22 and "null acc" in err()
        assert U(None, p, p, p, 1, 4, p, p, None) == -22 and "null pointer" in err()
        assert U(None, None, None, None, 0, 4, p, None, None) == 0
        assert F(None, p, 4, p, None, None) == -22 and "null pointer" in err()
        assert F(p, None, 4, p, C.c_void_p(host_addr(host) + 256), None) == -22 and "node2chrom" in err()
        assert F(p, p, 4, p, p, None) == -22 and "alias" in err()
        assert F(p, p, -4, p, None, None) == -22 and "n_nodes" in err()
        need = lib.matcha_block_colmax_workspace_bytes(70, 3)
        assert need == 1792 and lib.matcha_block_colmax_workspace_bytes(0, 3) == 0
        assert Nm(p, 70, p, 3, p, need - 1, None) == -22 and "too small" in err()
        assert Nm(p, 70, None, 3, p, need, None) == -22 and "null pointer" in err()
        assert Nm(p, 70, p, -1, p, need, None) == -22 and "n_ranges" in err()
        assert Nm(p, 70, None, 0, None, 0, None) == 0
    assert not log.counts


def host_addr(buf):
    return C.addressof(buf)


# ---- the host side of ClusterAdj ---------------------------------------------------------------------------------------------------------
def test_update_refusals_come_before_the_device():
    ca = PC.ClusterAdj(10, np.zeros(11, dtype=np.int32), device="cpu")         # nothing is allocated until an update is accepted
    with pytest.raises(ValueError, match="finite"):
        ca.update([[1, 2], [2, 3]], weight=[1.0, float("nan")])
    with pytest.raises(ValueError, match="finite"):
        ca.update([[1, 2]], weight=[float("inf")])
    with pytest.raises(ValueError, match="2 weights for 1"):
        ca.update([[1, 2]], weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="2\\^30"):
        ca.update([[1, 2, 3], [1, 4]], weight=[2.0 ** 29, 2.0 ** 29])          # 2^61 + 2^61 = 2^62
    with pytest.raises(ValueError, match="65535"):
        ca.update((np.ones(65536, dtype=np.int32), np.asarray([0, 65536])))
    with pytest.raises(ValueError, match="offsets"):
        ca.update((np.ones(4, dtype=np.int32), np.asarray([0, 3])))
    assert ca.q_abs_sum == 0 and ca.n_pairs == 0 and ca._acc is None
    with pytest.raises(_lib.MatchaHipError, match="no CPU fallback"):
        ca.update([[1, 2]], weight=[2.0 ** 29])                               # accepted by the host checks: now it needs the device
    with pytest.raises(_lib.MatchaHipError):
        ca.finish()
    assert ca.q_abs_sum == 0
    with pytest.raises(ValueError):
        PC.ClusterAdj(0, None)
    with pytest.raises(ValueError, match="cover"):
        PC.ClusterAdj(10, np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError, match="block_max"):
        PC.clusters_to_adj([[1, 2]], None, 4, normalise="max")
    with pytest.raises(ValueError, match="chrom_range"):
        PC.clusters_to_adj([[1, 2]], None, 4, normalise="block_max")
    with pytest.raises(_lib.MatchaHipError):
        PC.block_colmax_normalise_(torch.zeros(4, 4, dtype=torch.float64), [[0, 4]])
    ids, offsets = PC._clusters_csr([[1, 2, 3], [], [4, 9]])
    assert ids.dtype == np.int32 and ids.tolist() == [1, 2, 3, 4, 9] and offsets.tolist() == [0, 3, 3, 5]
    ids2, off2 = PC._clusters_csr((torch.tensor([1, 2, 3, 4, 9]), np.asarray([0, 3, 3, 5])))
    assert ids2.tolist() == ids.tolist() and off2.tolist() == offsets.tolist()


def _write_inputs(tmp_path, max_cluster_size=3):
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("chr1\t1000\nchr2\t600\n")
    lines = ["a\tchr1:10\tchr1:250\tchr2:120", "b\tchr1:10\tchr1:250", "c\tchr1:0\tchr1:100\tchr1:200\tchr1:300\tchr2:0\tchr2:500",
             "d\tchr2:120\tchr2:320\tchrX:5"]
    clusters = tmp_path / "clusters.txt"
    clusters.write_text("\n".join(lines) + "\n")
    temp = tmp_path / "temp"
    cfg = {"resolution": 100, "chrom_list": ["chr1", "chr2"], "temp_dir": str(temp), "chrom_size": str(sizes), "cluster_path": str(clusters),
           "max_cluster_size": max_cluster_size, "mcool_path": str(tmp_path / "none.mcool")}
    path = tmp_path / "config.JSON"
    path.write_text(json.dumps(cfg))
    return str(path), temp


def test_main_from_clusters_reaches_the_device_without_h5py(tmp_path):
    """--adj-from clusters: h5py is never imported, so its absence is no SystemExit; the dictionaries and edge_list.npy are written with the
    config's bound; without a GPU the run ends at the library's own error, with one it writes the two matrices."""
    config, temp = _write_inputs(tmp_path)
    argv = ["--config", config, "--adj-from", "clusters", "--adj-weight", "two_over_n", "--adj-max-cluster-size", "10"]
    if torch.cuda.is_available():
        PC.main(argv)
        intra, inter = np.load(temp / "intra_adj.npy"), np.load(temp / "inter_adj.npy")
        assert intra.shape == (18, 18) and inter.shape == (18, 18) and intra.dtype == np.float64
        q = lambda n: int(np.rint(2.0 / n * 2.0 ** 32))
        assert intra[0, 2] == intra[2, 0] == (q(3) + q(2) + q(6)) / 2.0 ** 32   # nodes 1 and 3: clusters a, b and c
        assert inter[0, 11] == inter[0, 16] == q(6) / 2.0 ** 32                 # cluster c (6 nodes) entered with the larger bound
        assert inter[0, 12] == q(3) / 2.0 ** 32 and intra[12, 14] == 1.0 and not np.diag(intra).any()
    else:
        with pytest.raises(_lib.MatchaHipError, match="no CPU fallback"):
            PC.main(argv)
    edge_list = np.load(temp / "edge_list.npy", allow_pickle=True)
    assert [list(e) for e in edge_list] == [[1, 3, 13], [1, 3], [13, 15]]      # max_cluster_size 3: cluster c is not in edge_list.npy
    assert np.load(temp / "chrom_range.npy").tolist() == [[1, 12], [12, 19]]


def test_mcool_stays_the_default_and_names_the_new_option(tmp_path, monkeypatch):
    config, _ = _write_inputs(tmp_path)
    monkeypatch.setitem(sys.modules, "h5py", None)                            # `import h5py` raises ImportError, installed or not
    with pytest.raises(SystemExit, match="--adj-from clusters"):
        PC.main(["--config", config])
    with pytest.raises(SystemExit):
        PC.main(["--config", config, "--adj-from", "hic"])


# ---- the host driver ---------------------------------------------------------------------------------------------------------------------
def test_host_driver_under_asan_ubsan():
    """tests/host/cluster_adj_checks, built by `make host-asan` with the other drivers and run stand-alone as tests/test_cpu_host_checks.py runs
    them: tri_unrank at every row boundary for s in {2, 3, 64, 65, 1000, 65535}, the pair count, every refusal, MATCHA_EHIP from the launches."""
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "cluster_adj_checks" in [w for line in f if line.startswith("HOST_DRIVERS") for w in line.split()]
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    run = subprocess.run([os.path.join(ROOT, "build", "host_asan", "cluster_adj_checks")], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert "ALL CLUSTER ADJACENCY HOST CHECKS PASSED" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
