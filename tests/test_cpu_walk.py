"""The hypergraph walk's tables and its numpy twin against the reference's own transition probabilities (tests/golden/walk_tiny.npz,
written by tools/make_walk_golden.py from the reference's alias tables), on the CPU.  The GPU kernel is held to the twin bit for bit in
tests/test_hip_walk.py; what the twin samples is held to the reference here."""
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, walk as Wk
from tests import sgns_cases as SC, walk_ref as WR
from tests.fp64_grade import K, tensor_err

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


# ---- the skip-gram cases of tests/sgns_cases.py: what the device comparisons of tests/test_hip_walk.py rest on, from the twin alone ----------
def _unchanged(c, p, table, rows):
    """Rows ``rows`` of table 0 (syn0) / 1 (syn1) are bit for bit the initial ones after pass p, in all three twins."""
    first = (c.syn0, c.syn1)[table]
    return all(np.array_equal(c.twins[k][p][table][rows], first[rows].astype(k[0])) for k in SC.DTYPES)


@pytest.mark.parametrize("d", SC.WIDTHS)
@pytest.mark.parametrize("name", ["A1", "A2"])
def test_dead_flanks_add_exact_zeros_in_every_twin(name, d):
    c = SC.case(name, d)
    x, ctr, y = (c.walks[:, i] for i in range(3))
    ids = set(c.walks.ravel().tolist())
    before = (c.syn0, c.syn1)
    for p, pairs in enumerate(c.trained):
        assert len(pairs) == 32 and [r[1:3] for r in pairs[:4]] == [(0, 1), (1, 0), (1, 2), (2, 1)]     # two contexts for every middle
        mid = [r for r in pairs if r[1] == 1]
        if name == "A1":                                         # one launch: no two middles may meet in a row
            drawn = sum((r[6] for r in mid), [])
            assert len(drawn) == 80 and len(set(drawn)) == 80 and not set(drawn) & ids
        else:                                                    # a launch per walk: a middle's own live draws are distinct rows
            own = other = 0
            for w in range(8):
                drawn = sum((r[6] for r in mid if r[0] == w), [])
                live = [t for t in drawn if t != ctr[w]]
                assert len(drawn) == 10 and len(set(live)) == len(live) and not set(live) & (set(x.tolist()) | set(y.tolist()))
                own += len(drawn) - len(live)
                other += len(set(live) & set(ctr.tolist()))
            print(f"{name} d={d}: {own} draws of the own centre, {other} of another walk's")
            assert own >= 2 and other >= 8
        # the flanks' margins hold on the tables the pass starts from and on those it leaves
        after = c.twins[SC.DTYPES[0]][p]
        for s0, s1 in (before, after):
            pos, neg = SC.flank_margins(c.walks, s0, s1, pairs)
            assert pos >= 40 and neg <= -100, (name, d, p, pos, neg)
        before = after
        assert _unchanged(c, p, 1, x) and _unchanged(c, p, 1, y) and _unchanged(c, p, 0, ctr)
        assert _unchanged(c, p, 0, 0) and _unchanged(c, p, 1, 0)
    # the middles did train: their centres' rows and every live draw moved in syn1, their contexts' rows in syn0
    s0, s1 = c.twins[SC.DTYPES[1]][0]
    moved0, moved1 = (np.flatnonzero((a != b).any(1)) for a, b in ((s0, c.syn0), (s1, c.syn1)))
    assert sorted(moved0.tolist()) == sorted(x.tolist() + y.tolist())
    live = {t for r in c.trained[0] if r[1] == 1 for t in r[6] if t != r[3]}
    assert sorted(moved1.tolist()) == sorted(live | set(ctr.tolist())) and (name != "A1" or len(moved1) == 88)


def test_wide_window_draws_from_the_slots_beside_the_window():
    c = SC.case("B", 64)
    pairs = c.trained[0]
    drawn = sum((r[6] for r in pairs), [])
    assert len(pairs) == 16 and len(drawn) == 80 and len(set(drawn)) == 80 and not set(drawn) & set(c.walks.ravel().tolist())
    assert {r[5] for r in pairs} == {1, 2, 3, 4, 5}                                # every reduced window; the context is in reach of each
    assert {r[2] - (r[1] - 5) for r in pairs} == {4, 6}                            # jj = window - 1, window + 1
    _, slots = WR.draws(8, 2, 0, c.noise, 5, 5, c.kw["seed"])
    assert all(slots[w * 2 + i, 1 + j - i].tolist() != ids for w, i, j, _, _, _, ids in pairs)   # window 1's slots (0, 2) hold other draws


def test_clipped_pairs_train_by_the_window_draw_alone():
    c = SC.case("C", 64)
    W, Lw = c.walks.shape
    valid = (c.walks >= 1) & (c.walks <= SC.N)
    assert W >= 16 and Lw == 6 and (valid.sum(1) == 2).all() and len(set(c.walks[valid].tolist())) == 2 * W
    assert {0, SC.N + 1} <= set(c.walks[~valid].tolist())
    places = {(int(np.flatnonzero(v)[0]), int(np.diff(np.flatnonzero(v))[0])) for v in valid}
    assert places == {(p, dist) for dist in (1, 2, 3) for p in (0, 5 - dist)} | {(2, 1), (1, 2), (1, 3)}     # start, mid-walk, end per dist
    pairs = c.trained[0]
    drawn = sum((r[6] for r in pairs), [])
    assert len(set(drawn)) == len(drawn) == 5 * len(pairs) and not set(drawn) & set(c.walks[valid].tolist())
    b_all, _ = WR.draws(W, Lw, 0, c.noise, 3, 5, c.kw["seed"])
    took = {(w, i) for w, i, *_ in pairs}
    idle = far = 0
    for w in range(W):
        p, q = np.flatnonzero(valid[w])
        for i in (p, q):
            assert ((w, i) in took) == (b_all[w * Lw + i] >= q - p)                # a position trains its partner iff b >= dist
            idle += (w, i) not in took
            far += (w, i) in took and q - p >= 2
    print(f"C: {len(pairs)} positions train ({far} at distance 2 or 3), {idle} have their partner out of reach")
    assert idle >= 2 and far >= 2 and idle + len(pairs) == 2 * W
    # the twin met bad ids, as centres and as contexts, and left every row but the pairs' and their draws' alone
    bad = []
    got = WR.sgns(c.walks, c.syn0, c.syn1, c.noise, n_nodes=SC.N, bad=bad, **c.kw)
    assert all(np.array_equal(a, b) for a, b in zip(got, c.twins[SC.DTYPES[0]][0]))
    assert any(i == j for _, i, j in bad) and any(i != j for _, i, j in bad)
    rows0, rows1 = ({r[k] for r in pairs} for k in (4, 3))
    for k in SC.DTYPES[1:]:
        s0, s1 = c.twins[k][0]
        assert set(np.flatnonzero((s0 != c.syn0).any(1)).tolist()) == rows0
        assert set(np.flatnonzero((s1 != c.syn1).any(1)).tolist()) == rows1 | set(drawn)


def _position_loop(c, mutant=None):
    """A float64 copy of the skip-gram position (the rule at the top of csrc/sgns.hip) over the case's passes, exact or with one branch
    broken -- the mutants the cases are there to catch: ``nocarry`` (a later context reads the centre's row as it was before the first),
    ``noreset`` (neu runs on from context to context), ``noskip`` (a draw of the centre itself is trained), ``jj_from_b`` (the negatives'
    slot counted from the reduced window)."""
    W, Lw = c.walks.shape
    kw = c.kw
    s0, s1 = c.syn0.astype(np.float64), c.syn1.astype(np.float64)
    for ep in c.epochs_run:
        g_base, g_total = ep * W * Lw, kw["epochs"] * W * Lw
        b_all, neg_all = WR.draws(W, Lw, g_base, c.noise, kw["window"], kw["negative"], kw["seed"])
        for w in range(W):
            for i in range(Lw):
                centre, g = int(c.walks[w, i]), g_base + w * Lw + i
                if c.n_nodes is not None and not 1 <= centre <= c.n_nodes:
                    continue
                lr = float(np.float32(max(kw["lr1"], kw["lr0"] - (kw["lr0"] - kw["lr1"]) * float(g) / float(g_total))))
                b = int(b_all[g - g_base])
                u0 = s1[centre].copy()
                u, neu = u0.copy(), np.zeros_like(u0)
                for j in range(max(0, i - b), min(Lw - 1, i + b) + 1):
                    ctx = int(c.walks[w, j])
                    if j == i or (c.n_nodes is not None and not 1 <= ctx <= c.n_nodes):
                        continue
                    v = s0[ctx].copy()
                    seen = u0 if mutant == "nocarry" else u
                    gt = (1.0 - 1.0 / (1.0 + np.exp(-(v @ seen)))) * lr
                    neu = gt * seen + (neu if mutant == "noreset" else 0.0)
                    u = u + gt * v
                    for t_id in neg_all[g - g_base, j - (i - (b if mutant == "jj_from_b" else kw["window"]))].tolist():
                        if t_id == centre and mutant != "noskip":
                            continue
                        t = s1[t_id].copy()
                        gt = (0.0 - 1.0 / (1.0 + np.exp(-(v @ t)))) * lr
                        neu = neu + gt * t
                        s1[t_id] = t + gt * v
                    s0[ctx] = s0[ctx] + neu
                s1[centre] = s1[centre] + (u - u0)
    return s0, s1


@pytest.mark.parametrize("mutant,name", [(None, "A1"), (None, "A2"), (None, "B"), (None, "C"), ("nocarry", "A1"), ("noreset", "A1"),
                                         ("noskip", "A2"), ("jj_from_b", "B"), ("jj_from_b", "C")])
def test_the_cases_tell_a_broken_position_from_the_twin(mutant, name):
    """The grade of tests/test_hip_walk.py (e <= K max(e(R32 seq), e(R32 tree), 2^-23) against the float64 twin) passes the exact position
    loop and misses each mutant by a factor of 10 at least on some table of the case meant for it: a condition on the inputs."""
    c = SC.case(name, 64)
    ratios = [tensor_err(g[:, c.cols], r[:, c.cols]) / n for g, r, n in zip(_position_loop(c, mutant), c.twins[SC.DTYPES[0]][-1], SC.noise_floor(c))]
    print(f"{name} {mutant}: e / noise syn0 {ratios[0]:.3g}, syn1 {ratios[1]:.3g}")
    if mutant is None:
        assert max(ratios) < K
    else:
        assert max(ratios) >= 10 * K
