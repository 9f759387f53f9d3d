"""The hypergraph walk's tables and its numpy twin against the reference's own transition probabilities (tests/golden/walk_tiny.npz,
written by tools/make_walk_golden.py from the reference's alias tables), on the CPU.  The GPU kernel is held to the twin bit for bit in
tests/test_hip_walk.py; what the twin samples is held to the reference here."""
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, walk as Wk
from tests import walk_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "walk_tiny.npz"))


@pytest.fixture(scope="module")
def graph(gold):
    return Wk.HyperWalkGraph(torch.from_numpy(gold["edges"]), int(gold["n_nodes"]), float(gold["p"]), float(gold["q"]))


def _pairs(gold):
    for i, (s, d) in enumerate(zip(gold["pair_src"].tolist(), gold["pair_dst"].tolist())):
        yield s, d, gold["second_p"][gold["second_ptr"][i]:gold["second_ptr"][i + 1]]


def test_fixture_is_the_graph_the_bounds_assume(gold, graph):
    """deg <= 100 (the 1e-8 bound's condition), an isolated node, a node with one incidence, one with more than 64, all three classes."""
    inc = np.diff(graph.inc_ptr.numpy())
    assert int(graph.deg.max()) <= 100 and inc[16] == 0 and inc[15] == 1 and inc.max() > 64
    seen = np.zeros(3, dtype=np.int64)
    for s, d, _ in _pairs(gold):
        seen += np.bincount(graph.classes(s, d, graph.transition(s, d)[0]), minlength=3)
    assert (seen > 0).all(), seen


def test_transition_matches_every_reference_distribution(gold, graph):
    worst = 0.0
    for v in range(1, int(gold["n_nodes"]) + 1):
        b, e = gold["first_ptr"][v - 1], gold["first_ptr"][v]
        ids, pr = graph.transition(None, v)
        assert ids.tolist() == gold["first_nb"][b:e].tolist()
        if len(ids):
            assert abs(pr.sum() - 1.0) < 1e-12
            worst = max(worst, float(np.abs(pr - gold["first_p"][b:e]).max()))
    n = 0
    for s, d, ref in _pairs(gold):
        ids, pr = graph.transition(s, d)
        assert ids.tolist() == graph.transition(None, d)[0].tolist() and len(ref) == len(ids)
        worst = max(worst, float(np.abs(pr - ref).max()))
        n += 1
    print(f"{n} ordered pairs, max abs difference {worst:.2e}")
    assert n == len(gold["pair_src"]) > 100 and worst <= 1e-8


def test_twin_samples_the_reference_distributions(gold, graph):
    """One fixed seed: for every ordered pair (src, dst) the twin visits n >= 2000 times, every cell of its empirical next-node distribution
    lies within 5 sqrt(p (1 - p) / n) of the reference's; at least 90 % of the pairs are visited that often."""
    N = int(gold["n_nodes"])
    walks, status = WR.walks(graph, num_walks=800, walk_length=80, seed=11)
    assert status.tolist() == [0, 0, 0, 0]
    a, b, c = (walks[:, i:walks.shape[1] - 2 + i].ravel().astype(np.int64) for i in range(3))
    cells = np.bincount((a * (N + 1) + b) * (N + 1) + c, minlength=(N + 1) ** 3).reshape(N + 1, N + 1, N + 1)
    qualified = total = 0
    for s, d, ref in _pairs(gold):
        total += 1
        row = cells[s, d]
        n = int(row.sum())
        ids = graph.transition(None, d)[0]
        assert row.sum() == row[ids].sum()                       # never a step to a non-neighbour
        if n < 2000:
            continue
        qualified += 1
        dev = np.abs(row[ids] / n - ref)
        assert (dev <= 5.0 * np.sqrt(ref * (1.0 - ref) / n)).all(), (s, d, n, dev.max())
    print(f"{qualified} of {total} ordered pairs visited >= 2000 times")
    assert qualified >= 0.9 * total
    # the first step: the first-order distribution
    for v in range(1, N + 1):
        ids, pr = graph.transition(None, v)
        got = np.bincount(walks[walks[:, 0] == v, 1], minlength=N + 1)
        n = int(got.sum())
        if len(ids):
            assert (np.abs(got[ids] / n - pr) <= 5.0 * np.sqrt(pr * (1.0 - pr) / n)).all(), v


@pytest.mark.parametrize("walk_length", [1, 2, 3, 9])
def test_twin_walks_are_walks(graph, walk_length):
    walks, status = WR.walks(graph, num_walks=7, walk_length=walk_length, seed=5)
    N = graph.n_nodes
    assert walks.shape == (7 * N, walk_length) and walks.dtype == np.int32 and status[1] == 0
    assert (walks[:, 0] == np.tile(np.arange(1, N + 1), 7)).all()              # walk w starts at nodes[w % n]
    nbr = {v: set(graph.transition(None, v)[0].tolist()) for v in range(1, N + 1)}
    for row in walks:
        for x, y in zip(row[:-1], row[1:]):
            assert (y in nbr[int(x)]) if nbr[int(x)] else (y == x)             # a neighbour; an isolated node repeats itself
    assert (walks[walks[:, 0] == 16] == 16).all()


def test_trial_cap_is_reported(graph):
    """max_trials = 1 and 2: the steps whose proposals were all refused keep the last one and are counted; the count falls with the cap."""
    w1, s1 = WR.walks(graph, 5, 10, seed=3, max_trials=1)
    w2, s2 = WR.walks(graph, 5, 10, seed=3, max_trials=2)
    wf, sf = WR.walks(graph, 5, 10, seed=3)
    assert s1[1] > s2[1] > 0 and sf[1] == 0 and s1[0] == s2[0] == 0
    assert (w1[:, :2] == w2[:, :2]).all() and (w1[:, :2] == wf[:, :2]).all()   # the first step has no acceptance test
    # with one trial a step is its first proposal: the first-order draw at (step, trial 0)
    nbr = {v: set(graph.transition(None, v)[0].tolist()) for v in range(1, 17)}
    assert all((y in nbr[int(x)]) if nbr[int(x)] else y == x for row in w1 for x, y in zip(row[:-1], row[1:]))


def test_thresholds():
    assert Wk.class_thresholds(2.0, 0.25) == [1 << 29, 1 << 30, 1 << 32]
    assert Wk.class_thresholds(0.25, 2.0) == [1 << 32, 1 << 30, 1 << 29]
    assert Wk.class_thresholds(1.0, 1.0) == [1 << 32] * 3
    assert Wk.class_thresholds(1.0, 3.0) == [1 << 32, 1 << 32, (1 << 32) // 3]
    with pytest.raises(ValueError):
        Wk.class_thresholds(0.0, 1.0)


def test_incidence_weights_and_subsets():
    edges = torch.tensor([[2, 5, 0, 0], [1, 2, 3, 4], [2, 3, 5, 0]])
    G = Wk.HyperWalkGraph(edges, 6)
    assert G.deg.tolist() == [0, 1, 3, 2, 1, 2, 0]
    assert G.inc_ptr.tolist() == [0, 0, 3, 9, 14, 17, 20, 20]
    assert G.inc_nb[G.inc_ptr[2]:G.inc_ptr[3]].tolist() == [5, 1, 3, 4, 3, 5]    # node 2: edges in input order, the other nodes ascending
    w = np.diff(G.inc_cum[3:9].numpy(), prepend=0)
    want = [round(2 ** 40 / (np.sqrt(dg) * k)) for dg, k in ((2, 2), (1, 4), (2, 4), (1, 4), (2, 3), (2, 3))]
    assert w.tolist() == want
    assert G.pairs.tolist() == [[1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [2, 5], [3, 4], [3, 5]]
    assert G.triples.tolist() == [[1, 2, 3], [1, 2, 4], [1, 3, 4], [2, 3, 4], [2, 3, 5]]
    assert Wk.HyperWalkGraph(torch.zeros((0, 3), dtype=torch.long), 4).inc_ptr.tolist() == [0] * 6


def test_refusals():
    with pytest.raises(ValueError, match="at most 8"):
        Wk.HyperWalkGraph(torch.arange(1, 10)[None, :], 20)
    with pytest.raises(ValueError, match="ascending"):
        Wk.HyperWalkGraph(torch.tensor([[3, 2, 0]]), 5)
    with pytest.raises(ValueError, match="ascending"):
        Wk.HyperWalkGraph(torch.tensor([[2, 2, 0]]), 5)
    with pytest.raises(ValueError, match="zero-padded"):
        Wk.HyperWalkGraph(torch.tensor([[0, 2, 3]]), 5)
    with pytest.raises(ValueError, match="node id outside"):
        Wk.HyperWalkGraph(torch.tensor([[2, 6, 0]]), 5)
    with pytest.raises(_lib.MatchaHipError):
        Wk.hyper_walks(Wk.HyperWalkGraph(torch.tensor([[1, 2]]), 2))        # a CPU graph: no CPU fallback
    with pytest.raises(ValueError, match="64, 128 or 256"):
        Wk.sgns_train(torch.zeros((1, 2), dtype=torch.int32), 4, 32)


def test_standard_scale_is_sklearns():
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(0)
    A = (rng.normal(size=(50, 6)) * [1, 10, 0.1, 3, 1, 1] + [0, 5, -2, 0, 0, 0]).astype(np.float32)
    A[:, 4] = 2.5                                                # a constant column divides by 1: all zeros
    got = Wk.standard_scale(torch.from_numpy(A)).numpy()
    want = StandardScaler().fit_transform(A.astype(np.float64))
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-6 and (got[:, 4] == 0).all()


def test_sgns_twin_learns_and_orders_agree():
    """The skip-gram twin itself: float32 in both summation orders stays at float32 distance from float64, and a pass lowers the loss."""
    rng = np.random.default_rng(1)
    N, d = 12, 64
    walks = rng.integers(1, N + 1, size=(6, 8)).astype(np.int32)
    syn0, syn1 = Wk.sgns_init(N, d, 7, device="cpu")
    assert float(syn0.abs().max()) <= 0.5 / d and (syn0[0] == 0).all() and (syn1 == 0).all() and len(np.unique(syn0[1:].numpy())) > 700
    noise = Wk.noise_table(torch.from_numpy(walks), N)
    cnt = np.bincount(walks.ravel(), minlength=N + 1).astype(np.float64)
    want = np.cumsum(np.rint(2.0 ** 32 * cnt ** 0.75 / (cnt ** 0.75).sum()))
    assert noise[0] == 0 and np.abs(noise.numpy() - want).max() <= 1 and abs(int(noise[-1]) - 2 ** 32) <= N
    kw = dict(window=3, negative=2, lr0=0.5, lr1=0.5, seed=7)
    a64 = WR.sgns(walks, syn0.numpy(), syn1.numpy(), noise.numpy(), **kw)
    a32 = WR.sgns(walks, syn0.numpy(), syn1.numpy(), noise.numpy(), dtype=np.float32, order="seq", **kw)
    b32 = WR.sgns(walks, syn0.numpy(), syn1.numpy(), noise.numpy(), dtype=np.float32, order="tree", **kw)
    for x, y in zip(a32 + b32, a64 + a64):
        assert x.dtype == np.float32 and np.abs(x - y).max() <= 1e-5 * np.abs(y).max()
    pairs = np.stack([walks[:, 1:].ravel(), walks[:, :-1].ravel()], 1)
    neg = rng.integers(1, N + 1, size=(len(pairs), 2))
    for _ in range(3):
        a64 = WR.sgns(walks, a64[0], a64[1], noise.numpy(), **kw)
    assert WR.sgns_loss(a64[0], a64[1], pairs, neg) < WR.sgns_loss(syn0.numpy(), syn1.numpy(), pairs, neg) - 0.05
