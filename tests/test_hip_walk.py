"""The hypergraph walk and the skip-gram pass on the device: hyper_walk_kernel bit for bit against the numpy twin
(tests/walk_ref.py; what the twin samples is held to the reference in tests/test_cpu_walk.py); sgns_kernel against the sequential twin where
no two positions meet in a row, at fp32 grade (the form of tests/fp64_grade.py: e <= 8 max(e(R32 seq), e(R32 tree), 2^-23) against the
float64 twin) -- one context per position on walks of length 2, and on the inputs of tests/sgns_cases.py several contexts, a window above
1, draws of the centre, bad ids in reach and one walk per launch -- and on a planted graph by what it learns; the chain
walk_embeddings -> train.run(table_init="walk") and the CLI's two files.  GPU only (-m gpu)."""
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, walk as Wk
from tests import sgns_cases as SC, walk_ref as WR
from tests.fp64_grade import K, ULP, tensor_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQ = [(2.0, 0.25), (0.25, 2.0), (1.0, 1.0)]


def synthetic_edges(n_nodes=300, n_edges=2000, seed=4):
    """n_edges distinct hyperedges of sizes 2 .. 8 over n_nodes nodes, zero-padded ascending, int64 [n_edges, 8]."""
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < n_edges:
        k = int(rng.integers(2, 9))
        rows.add(tuple(sorted((1 + rng.choice(n_nodes, size=k, replace=False)).tolist())))
    out = np.zeros((n_edges, 8), dtype=np.int64)
    for i, r in enumerate(sorted(rows)):
        out[i, :len(r)] = r
    return out[rng.permutation(n_edges)]


@pytest.fixture(scope="module")
def edge_lists():
    g = np.load(os.path.join(ROOT, "tests", "golden", "walk_tiny.npz"))
    return {"tiny": (g["edges"], int(g["n_nodes"])), "synth": (synthetic_edges(), 300)}


_graphs = {}


def graphs(edge_lists, name, p, q):
    """(the graph on the device, the twin's tables of the SAME graph built on the host) -- the tables must agree to begin with."""
    if (name, p, q) not in _graphs:
        edges, N = edge_lists[name]
        dev = Wk.HyperWalkGraph(torch.from_numpy(edges).cuda(), N, p, q)
        host = Wk.HyperWalkGraph(torch.from_numpy(edges), N, p, q)
        for f in ("inc_ptr", "inc_nb", "inc_cum", "pairs", "triples"):
            assert torch.equal(getattr(dev, f).cpu(), getattr(host, f)), f
        assert dev.thresholds == host.thresholds
        _graphs[(name, p, q)] = (dev, WR.Tables(host))
    return _graphs[(name, p, q)]


def both(edge_lists, name, p, q, nodes, num_walks, walk_length, seed, max_trials, **kw):
    dev, tables = graphs(edge_lists, name, p, q)
    got, st = Wk.hyper_walks(dev, num_walks, walk_length, seed, max_trials, nodes=nodes, **kw)
    want, st_want = WR.walks(tables, num_walks, walk_length, seed, max_trials, nodes=nodes)
    return got.cpu().numpy(), st.cpu().numpy(), want, st_want


@pytest.mark.parametrize("name", ["tiny", "synth"])
@pytest.mark.parametrize("p,q", PQ)
def test_walks_equal_the_twin_bit_for_bit(edge_lists, name, p, q):
    got, st, want, st_want = both(edge_lists, name, p, q, None, 3, 17, 21, 1024)
    assert got.dtype == np.int32 and got.shape == want.shape == (3 * edge_lists[name][1], 17)
    assert np.array_equal(got, want) and np.array_equal(st, st_want) and st[1] == 0
    assert len(np.unique(got[:, 2:])) > 10                      # (walks that go somewhere)


@pytest.mark.parametrize("walkers", [1, 63, 64, 65, 257])
def test_walker_counts(edge_lists, walkers):
    nodes = (1 + (np.arange(walkers) * 7) % 300).astype(np.int32)
    got, st, want, st_want = both(edge_lists, "synth", 2.0, 0.25, nodes, 1, 17, 5, 1024)
    assert got.shape == (walkers, 17) and np.array_equal(got, want) and np.array_equal(st, st_want)


@pytest.mark.parametrize("walk_length", [1, 2, 3, 17])
def test_walk_lengths(edge_lists, walk_length):
    for name in ("tiny", "synth"):
        got, st, want, st_want = both(edge_lists, name, 2.0, 0.25, None, 2, walk_length, 9, 1024)
        assert got.shape[1] == walk_length and np.array_equal(got, want) and np.array_equal(st, st_want)
    assert (got[:, 0] == np.tile(np.arange(1, 301), 2)).all()


@pytest.mark.parametrize("max_trials", [1, 2, 1024])
@pytest.mark.parametrize("p,q", PQ)
def test_trial_cap_and_status_words(edge_lists, max_trials, p, q):
    for name in ("tiny", "synth"):
        got, st, want, st_want = both(edge_lists, name, p, q, None, 2, 17, 13, max_trials)
        assert np.array_equal(got, want) and np.array_equal(st, st_want) and st[0] == 0
        # every class accepts always at p = q = 1; otherwise a cap of 1 or 2 is reached somewhere and the full cap nowhere
        assert (st[1] > 0) == (max_trials <= 2 and (p, q) != (1.0, 1.0)), (name, st)


def test_chunked_by_walk_range_equals_unchunked_and_is_logged(edge_lists):
    dev, tables = graphs(edge_lists, "synth", 2.0, 0.25)
    whole, st = Wk.hyper_walks(dev, 2, 17, 3)
    with _lib.launch_log() as log:
        parts, st_parts = Wk.hyper_walks(dev, 2, 17, 3, chunk_walks=129)
        torch.cuda.synchronize()
    assert torch.equal(whole, parts) and torch.equal(st, st_parts)
    assert log.counts.get("hyper_walk_kernel") == -(-600 // 129)
    want, _ = WR.walks(tables, 2, 17, 3)
    assert np.array_equal(whole.cpu().numpy(), want)


def test_isolated_and_foreign_starts(edge_lists):
    dev, _ = graphs(edge_lists, "tiny", 2.0, 0.25)
    got, st = Wk.hyper_walks(dev, 1, 5, 0, nodes=[16, 0, 3])
    assert got[0].tolist() == [16] * 5 and got[1].tolist() == [0] * 5 and st[0] == 0        # no incidences: the node repeats itself
    got, st = Wk.hyper_walks(dev, 1, 5, 0, nodes=[3, 17, -1])
    assert got[1].tolist() == [0] * 5 and got[2].tolist() == [0] * 5 and int(st[0]) & _lib.STATUS_BAD_ID


# ---- skip-gram -----------------------------------------------------------------------------------------------------------------------
RACE_FREE_SEED, RF_N = 1, 5000


@pytest.fixture(scope="module")
def race_free():
    """8 walks of length 2 over 16 distinct ids of 5000, a noise table that never draws a walk's id, window 1: position (w, 0) touches
    syn1[a], syn0[b] and its negatives' syn1 rows, position (w, 1) syn1[b], syn0[a] and its negatives' -- with all negatives of a pass
    distinct no two positions of a launch meet in a row, and the sequential twin is THE answer."""
    rng = np.random.default_rng(3)
    walks = rng.choice(np.arange(1, RF_N + 1), size=16, replace=False).reshape(8, 2).astype(np.int32)
    wts = np.full(RF_N + 1, round(2 ** 32 / (RF_N - 16)), dtype=np.int64)
    wts[0] = 0
    wts[walks.ravel()] = 0
    return walks, np.cumsum(wts)


def _tables(d, seed=0):
    rng = np.random.default_rng(100 + seed)
    return (rng.uniform(-0.5, 0.5, size=(RF_N + 1, d)).astype(np.float32), rng.uniform(-0.5, 0.5, size=(RF_N + 1, d)).astype(np.float32))


def _grade(label, got, r64, r32a, r32b, cols=None):
    """``cols`` (a mask): the error and max|r| over those columns only.  Returns the worst e / noise."""
    worst = 0.0
    for name, g, a, b, c in zip(("syn0", "syn1"), got, r64, r32a, r32b):
        if cols is not None:
            g, a, b, c = (t[:, cols] for t in (g, a, b, c))
        noise = max(tensor_err(b, a), tensor_err(c, a), ULP)
        err = tensor_err(g, a)
        print(f"{label} {name}: e {err:.2e}, noise {noise:.2e}, ratio {err / noise:.2f}")
        assert err <= K * noise, (label, name, err, noise)
        worst = max(worst, err / noise)
    return worst


@pytest.mark.parametrize("d", [64, 128, 256])
def test_sgns_without_races_matches_the_sequential_twin(race_free, d):
    walks, noise = race_free
    kw = dict(window=1, negative=5, lr0=0.025, lr1=1e-4, seed=RACE_FREE_SEED, epochs=2)
    s0, s1 = _tables(d)
    refs, touched = {}, []
    for dtype, order in ((np.float64, "seq"), (np.float32, "seq"), (np.float32, "tree")):
        a = (s0, s1)
        passes = []
        for ep in range(2):
            drawn = []
            a = WR.sgns(walks, a[0], a[1], noise, epoch=ep, dtype=dtype, order=order, drawn=drawn, **kw)
            passes.append(a)
            touched.append(drawn)
        refs[(dtype, order)] = passes
    for drawn in touched:                                        # the condition the comparison rests on
        assert len(drawn) == 80 and len(set(drawn)) == 80 and not set(drawn) & set(walks.ravel().tolist())
    wt, nt = torch.from_numpy(walks).cuda(), torch.from_numpy(noise).cuda()
    g0, g1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
    for ep in range(2):
        with _lib.launch_log() as log:
            st = Wk.sgns_epoch(wt, g0, g1, nt, epoch=ep, chunk_walks=8, **kw)          # ONE launch: all 16 positions at once
            torch.cuda.synchronize()
        assert log.counts.get("sgns_kernel") == 1 and st.tolist() == [0, 0, 0, 0]
        _grade(f"d={d} pass {ep}", (g0.cpu().numpy(), g1.cpu().numpy()), refs[(np.float64, "seq")][ep], refs[(np.float32, "seq")][ep],
               refs[(np.float32, "tree")][ep])
    # rows no position touched are bit for bit what they were
    rows = np.ones(RF_N + 1, dtype=bool)
    rows[walks.ravel()] = False
    rows[np.asarray(sum(touched, []))] = False
    assert np.array_equal(g0.cpu().numpy()[rows], s0[rows]) and np.array_equal(g1.cpu().numpy()[rows], s1[rows])
    changed = np.abs(g1.cpu().numpy() - s1).max(1) > 0
    assert changed.sum() >= 16 + 80                              # the centres and every negative of the first pass moved


def test_sgns_edge_forms(race_free):
    walks, noise = race_free
    s0, s1 = _tables(64, 1)
    wt, nt = torch.from_numpy(walks).cuda(), torch.from_numpy(noise).cuda()
    # negative = 0 and a window larger than the walk (b is drawn from 1 .. 7, every context in bounds is taken)
    kw = dict(window=7, negative=0, lr0=0.05, lr1=0.05, seed=2)
    g0, g1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
    assert Wk.sgns_epoch(wt, g0, g1, nt, chunk_walks=8, **kw).tolist() == [0, 0, 0, 0]
    r64 = WR.sgns(walks, s0, s1, noise, **kw)
    r32a = WR.sgns(walks, s0, s1, noise, dtype=np.float32, order="seq", **kw)
    r32b = WR.sgns(walks, s0, s1, noise, dtype=np.float32, order="tree", **kw)
    _grade("negative=0 window=7", (g0.cpu().numpy(), g1.cpu().numpy()), r64, r32a, r32b)
    assert (np.abs(g0.cpu().numpy() - s0).max(1) > 0).sum() == 16
    # walks of length 1: no context, nothing changes
    g0, g1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
    single = torch.from_numpy(np.ascontiguousarray(walks.reshape(16, 1))).cuda()
    assert Wk.sgns_epoch(single, g0, g1, nt, window=3, negative=5, seed=2, chunk_walks=16).tolist() == [0, 0, 0, 0]
    assert np.array_equal(g0.cpu().numpy(), s0) and np.array_equal(g1.cpu().numpy(), s1)
    # an id outside 1 .. N trains nothing and is flagged
    bad = torch.tensor([[3, RF_N + 1], [0, 4]], dtype=torch.int32).cuda()
    st = Wk.sgns_epoch(bad, g0, g1, nt, window=1, negative=0, seed=2)
    assert int(st[0]) & _lib.STATUS_BAD_ID and np.array_equal(g0.cpu().numpy(), s0) and np.array_equal(g1.cpu().numpy(), s1)


def _run_case(c, chunk_walks):
    """The case's passes on the device, on copies of its tables: per pass (syn0, syn1, the status words, the launches of sgns_kernel)."""
    wt, nt = torch.from_numpy(c.walks.copy()).cuda(), torch.from_numpy(c.noise.copy()).cuda()
    g0, g1 = torch.from_numpy(c.syn0.copy()).cuda(), torch.from_numpy(c.syn1.copy()).cuda()
    out = []
    for ep in c.epochs_run:
        with _lib.launch_log() as log:
            st = Wk.sgns_epoch(wt, g0, g1, nt, epoch=ep, chunk_walks=chunk_walks, **c.kw)
            torch.cuda.synchronize()
        out.append((g0.cpu().numpy(), g1.cpu().numpy(), st.tolist(), log.counts.get("sgns_kernel")))
    return out


def _check_case(c, passes):
    """Every pass at fp32 grade against the case's twins over its columns; the rows both float32 twins leave as they were (every column
    of them) are bit for bit as they were on the device."""
    worst = 0.0
    for p, (g0, g1, _, _) in enumerate(passes):
        r64, r32a, r32b = (c.twins[k][p] for k in SC.DTYPES)
        worst = max(worst, _grade(f"{c.name} d={c.d} pass {c.epochs_run[p]}", (g0, g1), r64, r32a, r32b, c.cols))
        for got, first, a, b in zip((g0, g1), (c.syn0, c.syn1), r32a, r32b):
            still = ~((a != first).any(1) | (b != first).any(1))
            assert still[0] and still.sum() >= SC.N - 200
            assert np.array_equal(got[still].view(np.uint32), first[still].view(np.uint32)), (c.name, c.d, p)
            assert ((got != first).any(1) == ~still).all()       # and every row the twins move moved
    print(f"{c.name} d={c.d}: worst e / noise {worst:.2f}")


@pytest.mark.parametrize("d", SC.WIDTHS)
def test_sgns_two_contexts_per_position_match_the_twin(d):
    """A1 (tests/sgns_cases.py): walks [x, c, y] whose flanks add exact zeros, all 24 positions in ONE launch, two passes: the carry of
    u from the first context to the second and the restart of neu, against the sequential twin."""
    c = SC.case("A1", d)
    passes = _run_case(c, chunk_walks=8)
    assert all(st == [0, 0, 0, 0] and launches == 1 for _, _, st, launches in passes)
    _check_case(c, passes)


@pytest.mark.parametrize("d", SC.WIDTHS)
def test_sgns_skips_its_own_centre_and_numbers_positions_across_launches(d):
    """A2: the same walks one per launch with the centres in the noise table, pass 1 of 4: a draw of the position's own centre is skipped,
    another walk's centre is a live row of an earlier or later launch, and g (the learning rate, the random stream) counts from the
    epoch's base plus the walk's offset in every launch."""
    c = SC.case("A2", d)
    passes = _run_case(c, chunk_walks=1)
    assert all(st == [0, 0, 0, 0] and launches == len(c.walks) == 8 for _, _, st, launches in passes)
    _check_case(c, passes)


@pytest.mark.parametrize("d", SC.WIDTHS)
def test_sgns_wide_window_draws_the_twins_negatives(d):
    """B: window 5 over walks of length 2 -- the negatives' slot jj = j - (i - window) -- in one launch, and bit for bit the same in
    launches of 3 walks (no two positions share a row, so chunking may not change a bit)."""
    c = SC.case("B", d)
    passes = _run_case(c, chunk_walks=8)
    assert all(st == [0, 0, 0, 0] and launches == 1 for _, _, st, launches in passes)
    _check_case(c, passes)
    (h0, h1, st, launches), = _run_case(c, chunk_walks=3)
    assert st == [0, 0, 0, 0] and launches == 3
    assert np.array_equal(h0.view(np.uint32), passes[0][0].view(np.uint32)) and np.array_equal(h1.view(np.uint32), passes[0][1].view(np.uint32))


@pytest.mark.parametrize("d", SC.WIDTHS)
def test_sgns_window_draw_clipping_and_bad_ids_among_the_contexts(d):
    """C: two valid ids per walk of 6 at distance 1 .. 3, at the walk's start, middle and end, among slots holding 0 and N + 1, window 3:
    a position trains its partner iff its drawn b reaches it, skips the bad slots in reach, and the call is flagged with nothing else."""
    c = SC.case("C", d)
    passes = _run_case(c, chunk_walks=len(c.walks))
    assert all(st == [_lib.STATUS_BAD_ID, 0, 0, 0] and launches == 1 for _, _, st, launches in passes)
    _check_case(c, passes)


@pytest.fixture(scope="module")
def planted():
    """4 disjoint communities of 32 nodes with 400 triples each; 10 walks of 20 nodes per node by the twin; a fixed evaluation set."""
    rng = np.random.default_rng(5)
    rows = []
    for c in range(4):
        s = set()
        while len(s) < 400:
            s.add(tuple(sorted((1 + 32 * c + rng.choice(32, 3, replace=False)).tolist())))
        rows += sorted(s)
    edges = np.asarray(rows, dtype=np.int64)
    N, d = 128, 64
    walks, _ = WR.walks(Wk.HyperWalkGraph(torch.from_numpy(edges), N), 10, 20, seed=1)
    syn0, syn1 = Wk.sgns_init(N, d, 1, "cpu")
    noise = Wk.noise_table(torch.from_numpy(walks), N)
    pairs = np.stack([walks[:, 1:].ravel(), walks[:, :-1].ravel()], 1).astype(np.int64)
    er = np.random.default_rng(9)
    pairs = pairs[er.choice(len(pairs), 2000, replace=False)]
    neg = er.integers(1, N + 1, size=(2000, 5))
    twin = WR.sgns(walks, syn0.numpy(), syn1.numpy(), noise.numpy(), window=3, seed=1)
    return dict(edges=edges, N=N, d=d, walks=walks, syn0=syn0, syn1=syn1, noise=noise, pairs=pairs, neg=neg, twin=twin)


def test_sgns_learns_the_planted_communities(planted):
    """The mean skip-gram loss over the evaluation set, by the twin in float64 from the tables: the kernel's pass must close at least half
    of the gap between the initial loss and the sequential twin's (atomics only reorder updates the twin makes in sequence; a kernel
    that does not learn, or moves the wrong rows, stays at the initial loss)."""
    P = planted
    walks_dev, _ = Wk.hyper_walks(Wk.HyperWalkGraph(torch.from_numpy(P["edges"]).cuda(), P["N"]), 10, 20, seed=1)
    assert np.array_equal(walks_dev.cpu().numpy(), P["walks"])
    g0, g1 = P["syn0"].cuda(), P["syn1"].cuda()
    assert torch.equal(Wk.sgns_init(P["N"], P["d"], 1, "cuda")[0], g0)
    with _lib.launch_log() as log:
        st = Wk.sgns_epoch(walks_dev, g0, g1, Wk.noise_table(walks_dev, P["N"]), window=3, seed=1)
        torch.cuda.synchronize()
    assert st.tolist() == [0, 0, 0, 0] and log.counts.get("sgns_kernel") == Wk.SGNS_MIN_LAUNCHES      # 1 280 walks: 64 launches of 20
    initial = WR.sgns_loss(P["syn0"].numpy(), P["syn1"].numpy(), P["pairs"], P["neg"])
    twin = WR.sgns_loss(P["twin"][0], P["twin"][1], P["pairs"], P["neg"])
    got = WR.sgns_loss(g0.cpu().numpy(), g1.cpu().numpy(), P["pairs"], P["neg"])
    print(f"skip-gram loss: initial {initial:.4f}, sequential twin {twin:.4f}, device {got:.4f}")
    assert twin < initial - 1.0 and got <= initial - 0.5 * (initial - twin)
    A = g0.cpu().numpy()[1:].astype(np.float64)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    cos, com = A @ A.T, np.arange(128) // 32
    for c in range(4):
        m = com == c
        within = (cos[np.ix_(m, m)].sum() - m.sum()) / (m.sum() * (m.sum() - 1))
        assert within > cos[np.ix_(m, ~m)].mean(), c
    assert (g0[0] == 0).all() and (g1[0] == 0).all()             # the padding row is no node


def test_walk_embeddings_are_standard_scaled(planted):
    P = planted
    table, walks, syn0 = Wk.walk_embeddings(torch.from_numpy(P["edges"]).cuda(), P["N"], 64, num_walks=10, walk_length=20, window=3, seed=1,
                                            return_parts=True)
    assert table.shape == (129, 64) and table.dtype == torch.float32 and (table[0] == 0).all()
    assert np.array_equal(walks.cpu().numpy(), P["walks"])
    body = table[1:].double()
    assert float(body.mean(0).abs().max()) < 1e-5 and float((body.pow(2).mean(0).sqrt() - 1).abs().max()) < 1e-5
    assert torch.allclose(table[1:], Wk.standard_scale(syn0[1:]))
