"""numpy twin of csrc/cluster_adj.hip: the same integer arithmetic -- q = rint(w 2^32) in float64, int64 sums over the
pairs of every accepted cluster, value = sum * 2^-32 -- so the device is compared with it for EQUALITY.  tests/test_cpu_cluster_adj.py shows the
twin equal, bit for bit, to the reference's own edgelist2adj / get_adjacency matrices (tests/golden/cluster_adj_tiny.npz)."""
import numpy as np

SCALE = float(1 << 32)


def weights_q(lens, weight):
    lens = np.asarray(lens, dtype=np.int64)
    if isinstance(weight, str):
        w = np.ones(len(lens)) if weight == "one" else 2.0 / np.maximum(lens, 1).astype(np.float64)
    else:
        w = np.asarray(weight, dtype=np.float64)
    return np.rint(w * SCALE).astype(np.int64)


def cluster_ok(c, n_nodes):
    c = np.asarray(c, dtype=np.int64)
    return len(c) >= 2 and c.min() >= 1 and c.max() <= n_nodes and (np.diff(c) > 0).all()


def acc_ref(clusters, n_nodes, weight="one"):
    """(acc int64 [N, N], upper triangle only; any cluster rejected).  Clusters of fewer than two nodes have no pairs."""
    q = weights_q([len(c) for c in clusters], weight)
    acc = np.zeros((n_nodes, n_nodes), dtype=np.int64)
    bad = False
    for c, qc in zip(clusters, q):
        if len(c) < 2:
            continue
        if not cluster_ok(c, n_nodes):
            bad = True
            continue
        c = np.asarray(c, dtype=np.int64) - 1
        i, j = np.triu_indices(len(c), k=1)
        np.add.at(acc, (c[i], c[j]), qc)
    return acc, bad


def finish_ref(acc, node2chrom=None):
    """The float64 matrix of an accumulator, mirrored with a zero diagonal; with node2chrom [N + 1] the pair (intra, inter)."""
    full = (acc + acc.T).astype(np.float64) * (1.0 / SCALE)
    np.fill_diagonal(full, 0.0)
    if node2chrom is None:
        return full
    n2c = np.asarray(node2chrom)[1:acc.shape[0] + 1]
    same = n2c[:, None] == n2c[None, :]
    return np.where(same, full, 0.0), np.where(same, 0.0, full)


def adj_ref(clusters, n_nodes, weight="one", node2chrom=None):
    return finish_ref(acc_ref(clusters, n_nodes, weight)[0], node2chrom)


def block_colmax_ref(A, ranges):
    """get_adjacency's normalisation on 0-based row blocks [lo, hi): A[lo:hi] /= A[lo:hi].max(axis=0) + 1e-10, in float64."""
    A = np.array(A, dtype=np.float64)
    for lo, hi in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
        if hi > lo:
            A[lo:hi, :] /= (np.max(A[lo:hi, :], axis=0, keepdims=True) + 1e-10)
    return A


def split_csr(ids, offsets):
    return [np.asarray(ids[offsets[c]:offsets[c + 1]]).tolist() for c in range(len(offsets) - 1)]
