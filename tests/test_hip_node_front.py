"""The node route of the table front end (model.hip, node_front_shape): when a step's token capacity B L + 1 is at least 4 (n_nodes + 1), x0, X
and the front end's backward run once per NODE and the encoder kernels gather their rows by node id.  Against the per-token route
(option disable_node_front) on the same batch: logits and losses bit for bit -- the forward computes the same values from the same rows --
and every gradient at fp32 grade against the fp64 oracle (tests/fp64_grade.py, K = 8), since the backward differs in summation order only.
The route itself is asserted from the launch log: node_scatter_kernel runs or does not.  GPU only (-m gpu).
"""
import contextlib

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.helpers import oracle_state
from tests.test_hip_model import hip_model, _trainer_grads

pytestmark = pytest.mark.gpu


def _no_dropout(clf):
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0


def _step(layout, sd, x, y, w, *, node, dropout, mode="table", seed=0, chrom=0, prepare=None, **trainer_kw):
    """One Trainer.forward_backward on a fresh model and Trainer with the node route allowed (``node``) or switched off.  Returns
    (logits, losses, gradients, kernels that ran, Trainer)."""
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS[layout], 64, mode, seed, sd=sd)
    if not dropout:
        _no_dropout(clf)
    clf.train()
    with (contextlib.nullcontext() if node else _lib.option("disable_node_front")):
        tr = Trainer(clf, lr=1e-3, base_seed=11, **trainer_kw)
        if prepare:
            prepare(tr)
        xd = torch.from_numpy(x).cuda().contiguous()
        yd = torch.from_numpy(y).cuda().contiguous()
        wd = torch.from_numpy(w).cuda().contiguous()
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xd, yd, wd, 1.0, 0.001, chrom)
            torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    grads = {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
    return logits.cpu().numpy().copy(), tr.losses.cpu().numpy().copy(), grads, ran, (tr, clf, xd)


def _eval_logits(layout, sd, x, *, node, seed=0):
    clf, _ = hip_model(synth.LAYOUTS[layout], 64, "table", seed, sd=sd)
    clf.eval()
    with (contextlib.nullcontext() if node else _lib.option("disable_node_front")), _lib.launch_log() as log, torch.no_grad():
        lg = clf(torch.from_numpy(x).cuda()).cpu().numpy().copy()
    return lg, log.counts


def _bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _table_name(grads):
    names = [n for n, g in grads.items() if g is not None and g.ndim == 2 and g.shape[1] == 64 and "embed" in n.lower()]
    assert len(names) == 1, names
    return names[0]


_C23 = {}


def _c23():
    """c23 (150 nodes, n_attr 24), 3 072 mixed-k rows, L = 5: capacity 15 361 > 13 824, so the large-batch kernels run, ~70 tokens per node."""
    if not _C23:
        num = synth.LAYOUTS["c23"]
        _, fe, sd = oracle_state(num, 64, "table", 71)
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5], 768, 571, 5)
        assert x.shape == (3072, 5)
        _C23.update(sd=sd, fe=fe, x=x, y=y, w=w, ref=G.references(sd, fe, x, y, w, chrom=0))      # the oracle's step: computed once, shared
    return _C23


def _routes_agree(layout, sd, fe, x, y, w, oracle=True, bad_id=False, ref=None):
    """The check of test 1 on one batch: dropout on -> logits and both losses bitwise equal between the routes; dropout-free -> every
    gradient of BOTH routes at fp32 grade against the fp64 oracle (``oracle`` False -- a batch the oracle cannot take, foreign ids --: the two
    routes against each other instead).  Returns the dropout-free gradients of (node route, per-token route)."""
    out = {}
    for node in (True, False):
        lg, ls, _, ran, (tr, _, _) = _step(layout, sd, x, y, w, node=node, dropout=True)
        assert ("node_scatter_kernel" in ran) == node, (node, sorted(ran))
        assert {"front_fwd3_kernel", "front_bwd_kernel", "fused_fwd32_kernel", "fused_bwdh_kernel"} <= ran, sorted(ran)
        if bad_id:
            with pytest.raises(IndexError):
                tr.check_status()
        else:
            tr.check_status()
        out[node] = (lg, ls)
    assert _bitwise(out[True][0], out[False][0])
    assert _bitwise(out[True][1], out[False][1]), (out[True][1], out[False][1])
    if oracle and ref is None:
        ref = G.references(sd, fe, x, y, w, chrom=0)
    grads = {}
    for node in (True, False):
        lg, ls, g, ran, _ = _step(layout, sd, x, y, w, node=node, dropout=False)
        assert ("node_scatter_kernel" in ran) == node, (node, sorted(ran))
        grads[node] = g
        out[node] = (lg, ls)
        if oracle:
            got = G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)
            G.assert_grade(f"{'node' if node else 'token'} route", G.grade(got, ref))
    assert _bitwise(out[True][0], out[False][0]) and _bitwise(out[True][1], out[False][1])
    if not oracle:
        # Same function of the same inputs, different summation order: the bound the repository's route-against-route tests use for that
        # (tests/test_hip_properties.py: 2e-5 of the tensor's largest element), since no oracle takes a foreign id
        for n, a in grads[True].items():
            b = grads[False][n]
            assert (a is None) == (b is None), n
            if a is not None and n != G.GAUGE:
                assert float(np.abs(a - b).max()) <= 2e-5 * float(np.abs(b).max()) + 1e-9, (n, float(np.abs(a - b).max()), float(np.abs(b).max()))
    return grads


def test_routes_agree():
    c = _c23()
    _routes_agree("c23", c["sd"], c["fe"], c["x"], c["y"], c["w"], ref=c["ref"])
    lg_n, cnt_n = _eval_logits("c23", c["sd"], c["x"], node=True)
    lg_t, cnt_t = _eval_logits("c23", c["sd"], c["x"], node=False)
    assert _bitwise(lg_n, lg_t)
    # an inference forward has no backward to tell the routes apart; both run the front end as one launch
    assert cnt_n.get("front_fwd3_kernel", 0) == 1 and cnt_t.get("front_fwd3_kernel", 0) == 1, (cnt_n, cnt_t)


def test_routes_agree_with_the_tail_backward_as_separate_kernels(monkeypatch):
    """loss_in_forward off: head_bwd_kernel reads the static branch's X rows too -- from the node table on the node route.  The workspace
    is poisoned first, so a row nobody wrote on this route cannot pass as a leftover of an earlier run."""
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")
    c = _c23()

    def nolif(tr):
        tr.loss_in_forward = False
    out = {}
    for node in (True, False):
        lg, ls, g, ran, _ = _step("c23", c["sd"], c["x"], c["y"], c["w"], node=node, dropout=False, prepare=nolif)
        assert ("node_scatter_kernel" in ran) == node and "head_bwd_kernel" in ran and "tail_bwd64_kernel" not in ran, sorted(ran)
        got = G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)
        G.assert_grade(f"{'node' if node else 'token'} route, separate tail", G.grade(got, c["ref"]))
        out[node] = (lg, ls)
    assert _bitwise(out[True][0], out[False][0]) and _bitwise(out[True][1], out[False][1])


def _took_node_route(layout, rows, *, mode="table", prepare=None, **trainer_kw):
    num = synth.LAYOUTS[layout]
    _, fe, sd = oracle_state(num, 64, mode, 72)
    per_k = rows // 4
    x, y, w = G.make_case_batch(layout, [2, 3, 4, 5], per_k, 572, 5)
    x, y, w = x[:rows], y[:rows], w[:rows]
    assert x.shape == (rows, 5), x.shape
    _, _, _, ran, _ = _step(layout, sd, x, y, w, node=True, dropout=True, mode=mode, seed=72, prepare=prepare, **trainer_kw)
    assert "fused_bwdh_kernel" in ran, sorted(ran)
    return "node_scatter_kernel" in ran


def test_size_rule_and_exclusions():
    # wide_adj as a table layout: N + 1 = 4 157, 4 (N + 1) = 16 628; capacities 16 501 (3 300 rows) and 17 001 (3 400 rows)
    assert int(np.sum(synth.LAYOUTS["wide_adj"])) + 1 == 4157
    assert not _took_node_route("wide_adj", 3300)
    assert _took_node_route("wide_adj", 3400)
    assert not _took_node_route("c23", 2048)                                  # the small-batch kernels
    assert _took_node_route("c23", 3072)
    assert not _took_node_route("c23", 3072, deterministic=True)

    def sparse(tr):
        tr._use_sparse = lambda B, L: True                                     # the row-sparse table gradient (opts.sparse_table_grad)
    assert not _took_node_route("c23", 3072, prepare=sparse)
    assert not _took_node_route("c23", 3072, mode="adj")
    assert _took_node_route("hg38_1mb", 4096)


def _id_batch(kind):
    c = _c23()
    rng = np.random.default_rng(573)
    x = c["x"].copy()
    if kind == "five":
        pool = np.array([3, 17, 64, 99, 150])
        for i in range(len(x)):
            k = int((x[i] != 0).sum())
            x[i, :k] = np.sort(rng.choice(pool, size=k, replace=False))
    elif kind == "foreign":
        rows = rng.choice(len(x), size=200, replace=False)
        x[rows[:100], 0] = 151 + rng.integers(0, 1000, size=100)               # past the table
        x[rows[100:], 0] = -1 - rng.integers(0, 1000, size=100)                # negative
    elif kind == "few":
        for i in range(len(x)):
            k = int((x[i] != 0).sum())
            x[i, :k] = np.sort(rng.choice(np.arange(1, 21), size=k, replace=False))
    return x


@pytest.mark.parametrize("kind", ["five", "foreign", "few"])
def test_ids(kind):
    c = _c23()
    x = _id_batch(kind)
    grads = _routes_agree("c23", c["sd"], c["fe"], x, c["y"], c["w"], oracle=kind != "foreign", bad_id=kind == "foreign")
    seen = np.zeros(151, dtype=bool)
    ok = (x >= 0) & (x <= 150)
    seen[x[ok]] = True
    seen[0] = False
    for node in (True, False):
        g = grads[node][_table_name(grads[node])]
        assert g.shape == (151, 64)
        assert float(np.abs(g[~seen]).max()) == 0.0, (kind, node)             # untouched nodes and row 0: exactly zero
        assert float(np.abs(g[seen]).max()) > 0.0


def test_sequences_on_one_workspace():
    """node-route step, per-token-route step, node-route step on ONE Trainer (one workspace, gradients re-zeroed in between) equal three
    fresh runs; dropout-free, so that the seed's position does not enter."""
    from matcha_amd.engine import Trainer
    c = _c23()
    sd, x, y, w = c["sd"], c["x"], c["y"], c["w"]
    fresh = {node: _step("c23", sd, x, y, w, node=node, dropout=False) for node in (True, False)}
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=sd)
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    for node in (True, False, True):
        tr.gflat.zero_()
        with (contextlib.nullcontext() if node else _lib.option("disable_node_front")), _lib.launch_log() as log:
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert (log.counts.get("node_scatter_kernel", 0) > 0) == node
        f_lg, f_ls, f_g, _, _ = fresh[node]
        assert _bitwise(lg.cpu().numpy(), f_lg) and _bitwise(tr.losses.cpu().numpy(), f_ls)
        for n, v in _trainer_grads(tr, clf).items():
            if v is None or n == G.GAUGE:
                continue
            a, b = v.cpu().double().numpy(), f_g[n]
            # the same kernels on the same inputs; only the float atomics' order differs from run to run (2e-5: see _routes_agree)
            assert float(np.abs(a - b).max()) <= 2e-5 * float(np.abs(b).max()) + 1e-9, (node, n)


def test_graph_replay_equals_eager():
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    with _lib.launch_log() as log:
        eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    assert log.counts.get("node_scatter_kernel", 0) == 1
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
