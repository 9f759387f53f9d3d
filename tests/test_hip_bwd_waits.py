"""The rotated walk of fused_bwdh_kernel's value-table instances and its eight unconditional per-node adds (fused_bwd.hip).
The adds are buffer atomics without a branch of their own: a row past the half tile's tokens gets an offset past the descriptor's range and the
hardware drops it; the staging of half tile t + 1 closes iteration t.  Neither changes a sum, and a dropped row reaches no row of the table:
against the same route with the sums formed by the token walk (option disable_node_dx) and against the deterministic route, on batches that
leave few, many or all-but-two rows of a half tile masked.

Shape: test_hip_node_v.py's (c23, 150 nodes, 3 072 mixed-k rows, L = 5: capacity 15 361 >= 64 x 151, so the value-table instance and the
per-node adds run); which body ran is read off the launch log and, as tests/test_hip_node_dx.py does, off the poisoned workspace (the dXs rows
are written exactly when the sums are NOT formed at the producers).  GPU only (-m gpu).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_node_dx import _compare, _got, _run
from tests.test_hip_node_front import _bitwise, _c23, _id_batch, _no_dropout, _step, _table_name

pytestmark = pytest.mark.gpu

KINDS = ["mixed", "all_k2", "all_k5", "single", "pads_and_empty", "five", "odd_rows", "l8"]


@pytest.fixture(autouse=True)
def _poisoned_workspace(monkeypatch):
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")


def _batch(kind):
    c = _c23()
    x, y, w = c["x"].copy(), c["y"], c["w"]
    rng = np.random.default_rng(591)
    if kind == "mixed":
        pass
    elif kind in ("all_k2", "all_k5"):
        k = 2 if kind == "all_k2" else 5
        x, y, w = G.make_case_batch("c23", [k], 3072, 592 + k, 5)
        assert x.shape == (3072, 5) and ((x != 0).sum(1) == k).all()
    elif kind == "single":                                     # ONE hyperedge of two nodes: one half tile, 30 masked rows adding 0.0 behind one key
        x[:] = 0
        x[1234, :2] = (17, 99)
    elif kind == "pads_and_empty":                             # pads anywhere inside the rows, a run of all-padding rows and scattered ones
        x = np.take_along_axis(x, np.argsort(rng.random(x.shape), axis=1), axis=1)
        x[200:330] = 0
        x[rng.choice(len(x), size=150, replace=False)] = 0
    elif kind == "five":                                       # five ids hold every token: ~2 000 adds per row of a replica
        x = _id_batch("five")
    elif kind == "odd_rows":
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5], 775, 594, 5)
        assert x.shape == (3100, 5)
    elif kind == "l8":                                         # the ML = 8 instance
        x, y, w = G.make_case_batch("c23", [2, 3, 5, 8], 384, 595, 8)
        assert x.shape == (1536, 8)
    else:
        raise KeyError(kind)
    assert x.shape[0] * x.shape[1] + 1 >= 64 * 151
    return x, y, w


def _dxs_written(tr, B, L):
    """tests/test_hip_node_dx.py's probe on the FIRST token row alone (the `single` batch has two tokens): did the forward store dXs rows per
    token into the poisoned workspace?"""
    ws, _ = tr._buffers(B, L)
    buf = C.create_string_buffer(8192)
    fn = tr.lib.matcha_debug_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_size_t]
    assert fn(C.byref(tr.rt.shape), B, L, buf, 8192) == 0
    off = dict((ln.split()[0], int(ln.split()[1])) for ln in buf.value.decode().strip().split("\n"))["dXs"]
    words = ws.view(torch.uint8)[off:off + 64 * 4].cpu().numpy().view(np.uint32)
    untouched = bool((words == 0xFFFFFFFF).all())
    assert untouched or bool(np.isfinite(words.view(np.float32)).all())
    return not untouched


RAN = {"node_r_kernel", "node_scatter_kernel", "tail_bwd64_kernel", "fused_fwd32_kernel", "fused_bwdh_kernel"}


@pytest.mark.parametrize("kind", KINDS)
def test_masked_adds_change_no_sum(kind):
    c = _c23()
    x, y, w = _batch(kind)
    lg, ls, g, ran, (tr, _, xd) = _run(True, c["sd"], x, y, w, dropout=False)
    tr.check_status()
    assert RAN <= ran, sorted(ran)
    assert not _dxs_written(tr, *xd.shape)                     # the sums were formed per node at the producers
    lg1, ls1, g1, ran1, (tr1, _, _) = _run(False, c["sd"], x, y, w, dropout=False)
    assert ran1 == ran and _dxs_written(tr1, *xd.shape)
    lg2, ls2, g2, ran2, _ = _step("c23", c["sd"], x, y, w, node=True, dropout=False, deterministic=True)
    assert "fused_bwdh_kernel" in ran2 and "fused_fwd32_kernel" in ran2, sorted(ran2)
    for a, b in ((lg1, ls1), (lg2, ls2)):
        assert _bitwise(lg, a) and _bitwise(ls, b), (kind, ls, b)
    assert np.isfinite(lg).all() and np.isfinite(ls).all()
    _compare(f"{kind}: adds in flight against the token walk", g, g1)
    ref = c["ref"] if kind == "mixed" else G.references(c["sd"], c["fe"], x, y, w, chrom=0)
    for label, gr in (("per-node adds", g), ("token walk", g1), ("deterministic", g2)):
        G.assert_grade(f"{kind}: {label}", G.grade(_got(lg, ls, gr), ref))
    # a masked add must never reach a foreign row: the table-gradient rows of nodes that are not in the batch are exactly zero
    table = g[_table_name(g)]
    absent = np.setdiff1d(np.arange(1, table.shape[0]), np.unique(x))
    assert kind not in ("single", "five") or len(absent) >= 145
    assert not table[absent].any(), (kind, absent[np.abs(table[absent]).max(1) > 0])


def _trainer(c):
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    return clf, Trainer(clf, lr=1e-3, base_seed=11)


@pytest.mark.parametrize("kind", ["mixed", "single"])
def test_three_optimiser_steps_on_a_poisoned_workspace(kind):
    c = _c23()
    x, y, w = _batch(kind)
    clf, tr = _trainer(c)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    seen = []
    for _ in range(3):
        with _lib.launch_log() as log:
            tr.step(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("fused_bwdh_kernel", 0) == 1 and log.counts.get("node_scatter_kernel", 0) == 1, log.counts
        assert not _dxs_written(tr, *xd.shape)
        assert np.isfinite(tr.losses.cpu().numpy()).all()
        assert all(bool(torch.isfinite(p).all()) for p in clf.parameters())
        clf.eval()
        with torch.no_grad():
            seen.append(clf(xd).cpu().numpy().copy())
        clf.train()
        assert np.isfinite(seen[-1]).all()
    assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])      # the weights did move


def test_graph_replay_equals_eager():
    c = _c23()
    clf, tr = _trainer(c)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))

    def grads():
        return {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
    eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    torch.cuda.synchronize()
    assert not _dxs_written(tr, *xd.shape)
    g_eager = grads()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
    out.zero_()
    tr.gflat.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
    _compare("one replay against eager", grads(), g_eager)
