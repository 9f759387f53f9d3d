"""Contact matrices from the clusters on the device (matcha_amd/process.py's ClusterAdj / clusters_to_adj, csrc/cluster_adj.hip).
Both sides of every comparison of matrices here sum integers (the device in int64 fixed point, the twin tests/cluster_adj_ref.py likewise, the
reference's matrices with integer weights), so every such comparison is EQUALITY.  tests/test_cpu_cluster_adj.py ties the twin to the reference's
own edgelist2adj / get_adjacency (tests/golden/cluster_adj_tiny.npz)."""
import math

import numpy as np
import pytest
import torch

from matcha_amd import _lib
from matcha_amd import features as F
from matcha_amd import process as PC
from oracle import hypersagnn as O
from tests import cluster_adj_ref as R
from tests.helpers import gold

pytestmark = pytest.mark.gpu
KERNELS = ("cluster_pairs_update_kernel", "cluster_adj_finish_kernel", "block_colmax_normalise_kernel")


@pytest.fixture(scope="module")
def g():
    return gold("cluster_adj_tiny.npz")


@pytest.fixture(scope="module")
def golden_clusters(g):
    return R.split_csr(g["ids"], g["offsets"])


def device_adj(clusters, N, weight="one", node2chrom=None, split=False):
    ca = PC.ClusterAdj(N, node2chrom).update(clusters, weight)
    out = ca.finish(split=split)
    st = ca.status()
    if split:
        return out[0].cpu().numpy(), out[1].cpu().numpy(), st
    return out.cpu().numpy(), st


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_golden_graph_gives_the_reference_matrices(g, golden_clusters):
    N = int(g["n_nodes"])
    with _lib.launch_log() as log:
        one, st = device_adj((g["ids"], g["offsets"]), N)                      # the (ids, offsets) form
        w, _ = device_adj(golden_clusters, N, g["weights"])                    # the list form
        norm = PC.clusters_to_adj(golden_clusters, None, N, weight=g["weights"], normalise="block_max", chrom_range=g["chrom_range"],
                                  split=False).cpu().numpy()
    assert st == [0, 0, 0, 0]
    assert same_bits(one, g["edgelist2adj"])                                   # edgelist2adj, float64
    assert same_bits(w.astype(np.float32), g["adjacency"])                     # get_adjacency(norm=False) returns float32
    assert same_bits(norm.astype(np.float32), g["adjacency_norm"])             # get_adjacency(norm=True)
    assert same_bits(norm, R.block_colmax_ref(R.adj_ref(golden_clusters, N, g["weights"]), g["chrom_range"] - 1))
    assert one[3, 32] == one[32, 3] >= 7.0 and not one[69].any() and not one[:, 69].any()
    # the three new kernels, for the calls that ran them: three updates, three finishes, one normalisation
    assert {k: log.counts.get(k, 0) for k in KERNELS} == dict(zip(KERNELS, (3, 3, 1)))
    intra, inter, st = device_adj(golden_clusters, N, "one", g["node2chrom"], split=True)
    ri, re = R.adj_ref(golden_clusters, N, "one", g["node2chrom"])
    assert same_bits(intra, ri) and same_bits(inter, re) and st[0] == 0
    assert same_bits(intra + inter, one) and not (intra * inter).any() and inter.any()
    assert not np.diag(intra).any() and not np.diag(inter).any() and not np.diag(one).any()
    # the one-shot form with the split, and the split of the normalised matrix
    ci, ce = PC.clusters_to_adj(golden_clusters, g["node2chrom"], N)
    assert same_bits(ci.cpu().numpy(), ri) and same_bits(ce.cpu().numpy(), re)
    ni, ne = PC.clusters_to_adj(golden_clusters, g["node2chrom"], N, weight=g["weights"], normalise="block_max", chrom_range=g["chrom_range"])
    ni, ne = ni.cpu().numpy(), ne.cpu().numpy()
    n2c = g["node2chrom"][1:]
    same = n2c[:, None] == n2c[None, :]
    assert same_bits(np.where(same, norm, 0.0), ni) and same_bits(np.where(same, 0.0, norm), ne)


def test_one_large_cluster_is_all_ones():
    """The unrank test: 44 850 pairs of ONE cluster, cut into 64-rank runs of hundreds of wavefronts."""
    N = 300
    A, st = device_adj([list(range(1, N + 1))], N)
    assert st[0] == 0 and np.array_equal(A, 1.0 - np.eye(N))


def test_mixed_sizes_start_runs_inside_every_kind_of_cluster():
    rng = np.random.default_rng(5)
    N = 257
    clusters = [sorted(rng.choice(np.arange(1, N + 1), size=s, replace=False).tolist()) for s in (2, 3, 63, 64, 65, 129) for _ in range(3)]
    clusters += [sorted(rng.choice(np.arange(1, N + 1), size=2, replace=False).tolist()) for _ in range(5000)]
    clusters = [clusters[i] for i in rng.permutation(len(clusters))]
    n2c = np.concatenate([[-1], np.repeat([0, 1, 2, 3], [64, 65, 1, 127])]).astype(np.int32)
    intra, inter, st = device_adj(clusters, N, "one", n2c, split=True)
    ri, re = R.adj_ref(clusters, N, "one", n2c)
    assert st[0] == 0 and same_bits(intra, ri) and same_bits(inter, re)
    # clusters without pairs in between (sizes 0 and 1) are passed over, wherever they stand
    holes = []
    for i, c in enumerate(clusters[:400]):
        holes += [c] + ([[]] * (i % 3) if i % 2 else [[int(c[0])]] * 70 if i == 100 else [])
    A, st = device_adj(holes, N)
    assert st[0] == 0 and same_bits(A, R.adj_ref(holes, N))


def test_one_pair_in_20000_clusters():
    A, st = device_adj([[1, 2]] * 20000, 5)
    want = np.zeros((5, 5))
    want[0, 1] = want[1, 0] = 20000.0
    assert st[0] == 0 and np.array_equal(A, want)


def test_empty_list_and_one_cluster():
    N = 9
    A, st = device_adj([], N)
    assert st == [0, 0, 0, 0] and A.shape == (N, N) and not A.any()
    A, st = device_adj([[2, 9]], N, weight=[3.0])
    want = np.zeros((N, N))
    want[1, 8] = want[8, 1] = 3.0
    assert st[0] == 0 and np.array_equal(A, want)
    i1, e1, _ = device_adj([[4]], N, "one", np.zeros(N + 1, dtype=np.int32), split=True)
    assert not i1.any() and not e1.any()


def test_streaming_and_order_do_not_change_a_bit(g, golden_clusters):
    """The reproducibility claim, with weights whose float sums WOULD depend on the order."""
    N = int(g["n_nodes"])
    rng = np.random.default_rng(11)
    w = rng.random(len(golden_clusters)) * 3.0 + 1e-3
    whole = PC.ClusterAdj(N, g["node2chrom"]).update(golden_clusters, w)
    half = len(golden_clusters) // 2
    parts = PC.ClusterAdj(N, g["node2chrom"]).update(golden_clusters[:half], w[:half]).update(golden_clusters[half:], w[half:])
    perm = rng.permutation(len(golden_clusters))
    shuffled = PC.ClusterAdj(N, g["node2chrom"]).update([golden_clusters[i] for i in perm], w[perm])
    assert torch.equal(whole._acc, parts._acc) and torch.equal(whole._acc, shuffled._acc)
    assert whole.q_abs_sum == parts.q_abs_sum == shuffled.q_abs_sum
    assert whole.n_pairs == parts.n_pairs == shuffled.n_pairs == sum(len(c) * (len(c) - 1) // 2 for c in golden_clusters)
    acc, _ = R.acc_ref(golden_clusters, N, w)
    assert np.array_equal(whole._acc.cpu().numpy(), acc) and not np.tril(acc).any()
    for a, b in zip(whole.finish(), shuffled.finish()):
        assert torch.equal(a, b)
    for a, b in zip(whole.finish(), R.finish_ref(acc, g["node2chrom"])):
        assert same_bits(a.cpu().numpy(), b)


def test_two_over_n_against_the_twin_and_the_true_sums(g, golden_clusters):
    N = int(g["n_nodes"])
    A, st = device_adj(golden_clusters, N, "two_over_n")
    assert st[0] == 0 and same_bits(A, R.adj_ref(golden_clusters, N, "two_over_n"))
    terms = {}
    for c in golden_clusters:
        for i in range(len(c)):
            for j in range(i + 1, len(c)):
                terms.setdefault((c[i] - 1, c[j] - 1), []).append(2.0 / len(c))
    hit = np.zeros((N, N), dtype=bool)
    for (i, j), t in terms.items():
        true = math.fsum(t)
        bound = len(t) * 2.0 ** -33 + 2.0 ** -52 * true      # each add is rounded once to 2^-32; fsum and 2/n round in float64
        assert abs(A[i, j] - true) <= bound and A[j, i] == A[i, j]
        hit[i, j] = hit[j, i] = True
    assert not A[~hit].any()


def test_bad_clusters_add_nothing_and_are_reported():
    """Rejected by the kernel's own checks -- small clusters (judged by the lanes of one step) and large ones (scanned by the wavefront): a
    descending pair, a repeated id, id 0, id N + 1, a negative id.  The other clusters' cells are unchanged and nothing is indexed out of bounds."""
    rng = np.random.default_rng(3)
    N = 200
    good = [sorted(rng.choice(np.arange(1, N + 1), size=s, replace=False).tolist()) for s in (2, 3, 5, 12, 40, 150, 2, 7) for _ in range(6)]
    big = list(range(1, 181))
    swapped = big[:90] + [92, 91] + big[92:]                                  # one descending pair in the middle of 180 ids
    bad = [[5, 3], [3, 9, 7], [4, 4, 8], [0, 6], [0, 1, 2, 3, 4, 5, 6], [7, N + 1], [2, 11, 12, 13, N + 1], [-3, 4], swapped, big[:-1] + [N + 1],
           [0] + big[1:], [2 ** 31 - 1, 5], [1, 2 ** 31 - 1]]
    mixed = list(good)
    for k, c in enumerate(bad):
        mixed.insert(3 * k + 1, c)
    want = R.adj_ref(good, N)
    assert R.acc_ref(mixed, N)[1] and same_bits(R.adj_ref(mixed, N), want)
    A, st = device_adj(mixed, N)
    assert st[0] & _lib.STATUS_BAD_ID and same_bits(A, want)
    for c in bad:                                                             # each kind on its own, and alone in its launch
        A, st = device_adj([good[0], c, good[1]], N)
        assert st[0] & _lib.STATUS_BAD_ID and same_bits(A, R.adj_ref(good[:2], N)), c
        A, st = device_adj([c], N)
        assert st[0] & _lib.STATUS_BAD_ID and not A.any(), c
    A, st = device_adj(good, N)
    assert st[0] == 0 and same_bits(A, want)


@pytest.mark.parametrize("N,blocks", [(70, (30, 25, 15)), (257, (1, 64, 65, 127)), (257, (127, 65, 64))])
def test_block_colmax_normalise_equals_numpy(N, blocks):
    rng = np.random.default_rng(N + len(blocks))
    A = rng.gamma(2.0, 3.0, size=(N, N)) * (rng.random((N, N)) < 0.7)
    A[:, 5] = 0.0                                                              # 0 / (0 + 1e-10)
    A[:, 6] = -rng.random(N)                                                   # a negative maximum
    A[3, 7] = 1e300
    edges = np.concatenate([[0], np.cumsum(blocks)])
    ranges = np.stack([edges[:-1], edges[1:]], axis=1)                         # (257, (127, 65, 64)) leaves the last row out of every block
    want = R.block_colmax_ref(A, ranges)
    t = torch.from_numpy(A.copy()).cuda()
    with _lib.launch_log() as log:
        got = PC.block_colmax_normalise_(t, ranges)
    assert got is t and log.counts == {"block_colmax_normalise_kernel": 1}
    assert same_bits(t.cpu().numpy(), want)
    if edges[-1] < N:
        assert same_bits(t.cpu().numpy()[edges[-1]:], A[edges[-1]:])
    with pytest.raises(ValueError, match="overlap"):
        PC.block_colmax_normalise_(t, [[0, 10], [9, 20]])
    with pytest.raises(ValueError, match="lo <= hi"):
        PC.block_colmax_normalise_(t, [[0, N + 1]])


def test_end_to_end_features_match_the_oracle(g, golden_clusters):
    """clusters_to_adj -> corrcoef_features + zscore_rows_ against the oracle's features of the twin's matrices, at the tolerances of
    tests/test_process_features.py (corrcoef: 2e-6 absolute; z-score: rtol 2e-5, atol 2e-6, same zero pattern).  The weight is
    edgelist2adj's ("one"): on this small graph several inter rows hold one value repeated, for which the z-score is 0 / 0.  Integer values
    have an exact float32 mean, so the float32 oracle and the float64 kernel both give NaN -> 0 there; with 2 / n weights the oracle's float32
    mean is off by an ulp and it returns +-1 for such a row, which is its rounding noise and not a property of the matrices."""
    N = int(g["n_nodes"])
    intra, inter = PC.clusters_to_adj(golden_clusters, g["node2chrom"], N)
    ri, re = R.adj_ref(golden_clusters, N, "one", g["node2chrom"])
    feats = F.corrcoef_features(intra, g["chrom_range"])
    ref = O.corrcoef_features(ri.astype(np.float32), g["chrom_range"])
    assert len(feats) == len(ref) == 3
    for f, r in zip(feats, ref):
        f = f.cpu().numpy()
        assert f.shape == r.shape and np.abs(f - r).max() <= 2e-6
    z = F.zscore_rows_(inter.to(torch.float32).contiguous()).cpu().numpy()
    zr = O.zscore_inter(re.astype(np.float32))
    assert np.allclose(z, zr, rtol=2e-5, atol=2e-6) and ((z != 0) == (zr != 0)).all() and (zr != 0).any()


def test_edgelist2adj_writes_the_reference_file(tmp_path, g, golden_clusters):
    arr = np.empty(len(golden_clusters), dtype=object)
    for i, c in enumerate(golden_clusters):
        arr[i] = c
    np.save(tmp_path / "edge_list.npy", arr, allow_pickle=True)
    np.save(tmp_path / "chrom_range.npy", g["chrom_range"])
    out = PC.edgelist2adj(str(tmp_path))
    saved = np.load(tmp_path / "edge_list_adj.npy")
    assert same_bits(saved, g["edgelist2adj"]) and same_bits(out, saved)
