"""The packed row order of the fused d = 64 step's plan (ragged.hip; DESIGN.md 3, "Packed row order"; switch disable_row_pack): rows ordered by size class so that
the greedy packer's half tiles fill to 31 tokens.  Against the same step in batch order, in one process: the plan's arrays and row_src equal the
NumPy twin (tests/row_pack_ref.py) bit for bit; logits and both losses are BITWISE equal, dropout on and in eval (a token's forward depends on its
own hyperedge alone, the dropout counters are keyed by the original slot, row_loss lives at the batch row); every gradient is a token-contracted
sum added in another order: within 2e-5 of its tensor's largest element, and at the fp64 oracle's grade (K = 8) under both settings; the launches
and the status word are the same.

Shapes: c23 (150 nodes), 3 072 rows of L = 5 (tests/test_hip_bwd_waits.py's: the value-table instance and the per-node adds run), 3 100 rows, and
1 536 rows of L = 8.  The workspace starts as NaN bytes.  GPU only (-m gpu)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests import row_pack_ref as R
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_launch_pairs import _plan
from tests.test_hip_node_dx import _got
from tests.test_hip_node_front import _bitwise, _c23, _id_batch, _no_dropout
from tests.test_hip_node_r import _close

pytestmark = pytest.mark.gpu

KINDS = ["mixed", "all_k2", "all_k5", "single", "pads_and_empty", "five", "foreign", "odd_rows", "l8"]
NODE_RAN = {"row_count_kernel", "row_scan_kernel", "row_fill_kernel", "node_r_kernel", "node_scatter_kernel", "tail_bwd64_kernel", "fused_fwd32_kernel",
            "fused_bwdh_kernel"}


@pytest.fixture(autouse=True)
def _poisoned_workspace(monkeypatch):
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")


def _setting(pack):
    return contextlib.nullcontext() if pack else _lib.option("disable_row_pack")


def _batch(kind):
    c = _c23()
    x, y, w = c["x"].copy(), c["y"], c["w"]
    rng = np.random.default_rng(601)
    if kind == "mixed":
        pass
    elif kind in ("all_k2", "all_k5"):
        k = 2 if kind == "all_k2" else 5
        x, y, w = G.make_case_batch("c23", [k], 3072, 602 + k, 5)
        assert x.shape == (3072, 5) and ((x != 0).sum(1) == k).all()
    elif kind == "single":                                     # ONE hyperedge of two nodes among all-padding rows
        x[:] = 0
        x[1234, :2] = (17, 99)
    elif kind == "pads_and_empty":                             # pads anywhere inside the rows, a run of all-padding rows and scattered ones
        x = np.take_along_axis(x, np.argsort(rng.random(x.shape), axis=1), axis=1)
        x[200:330] = 0
        x[rng.choice(len(x), size=150, replace=False)] = 0
    elif kind in ("five", "foreign"):                          # five ids hold every token; ids outside the table
        x = _id_batch(kind)
    elif kind == "odd_rows":
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5], 775, 604, 5)
        assert x.shape == (3100, 5)
    elif kind == "l8":
        x, y, w = G.make_case_batch("c23", [2, 3, 5, 8], 384, 605, 8)
        assert x.shape == (1536, 8)
    else:
        raise KeyError(kind)
    return x, y, w


def _layout(tr, B, L):
    buf = C.create_string_buffer(8192)
    fn = tr.lib.matcha_debug_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_size_t]
    assert fn(C.byref(tr.rt.shape), B, L, buf, 8192) == 0
    return dict((ln.split()[0], int(ln.split()[1])) for ln in buf.value.decode().strip().split("\n"))


def _row_src(tr, ws, B, L):
    off = _layout(tr, B, L)["row_src"]
    return ws.view(torch.uint8)[off:off + 4 * B].cpu().numpy().view(np.int32).copy()


def _grads(tr, clf):
    return {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}


def _run(pack, x, y, w, *, dropout, node=True, mode="table", sd=None, seed=0, chrom=0, **trainer_kw):
    """One Trainer.forward_backward on a fresh model and Trainer under one setting of the switch."""
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, mode, seed, sd=_c23()["sd"] if sd is None else sd)
    if not dropout:
        _no_dropout(clf)
    clf.train()
    with _setting(pack), (contextlib.nullcontext() if node else _lib.option("disable_node_front")):
        tr = Trainer(clf, lr=1e-3, base_seed=11, **trainer_kw)
        xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xd, yd, wd, 1.0, 0.001, chrom)
            torch.cuda.synchronize()
    ws, _ = tr._buffers(*x.shape)
    return dict(lg=logits.cpu().numpy().copy(), ls=tr.losses.cpu().numpy().copy(), g=_grads(tr, clf), counts={k: n for k, n in log.counts.items() if n > 0},
                plan=_plan(ws, *x.shape), row_src=_row_src(tr, ws, *x.shape), status=tr.rt.status.cpu().numpy().copy())


def _eval(pack, x):
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=_c23()["sd"])
    clf.eval()
    with _setting(pack), _lib.launch_log() as log, torch.no_grad():
        lg = clf(torch.from_numpy(x).cuda()).cpu().numpy().copy()
    return lg, {k: n for k, n in log.counts.items() if n > 0}


def _plan_equals_twin(label, x, got, packed, n_nodes=150):
    """Every array of the plan a later kernel reads, and row_src, against the twin."""
    B, L = x.shape
    want = R.plan(x, n_nodes, packed=packed)
    Tr = want["tokens"]
    cnt = got["plan"]["count"].view(np.int32)
    assert (cnt[0], cnt[1], cnt[2], cnt[3]) == (Tr + 1, Tr, 0, want["halves"]), (label, cnt, Tr, want["halves"])
    view = lambda n, dt: got["plan"][n].view(dt)
    assert np.array_equal(view("row_off", np.int32), want["row_off"]), label
    for n, dt in (("tok_slot", np.int32), ("tok_id", np.int64), ("tok_pos", np.int32)):
        assert np.array_equal(view(n, dt)[:Tr + 1], want[n][:Tr + 1]), (label, n)
    assert np.array_equal(view("tok_key", np.int32), want["tok_key"]), label
    hm = view("half_meta", np.int32).reshape(-1, 4)
    assert np.array_equal(hm[:want["halves"]], want["half_meta"]) and not hm[want["halves"]:].any(), label
    if packed:
        assert np.array_equal(got["row_src"], want["row_src"]), label
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_packed_step_against_batch_order(kind):
    c = _c23()
    x, y, w = _batch(kind)
    on, off = (_run(p, x, y, w, dropout=True) for p in (True, False))
    assert NODE_RAN <= on["counts"].keys(), sorted(on["counts"])            # the five-launch plan, the value-table instance and the per-node adds ran
    assert on["counts"] == off["counts"], (on["counts"], off["counts"])      # no launch added, none renamed
    new = _plan_equals_twin(f"{kind}: packed", x, on, True)
    old = _plan_equals_twin(f"{kind}: batch order", x, off, False)
    print(f"{kind}: tokens {new['tokens']}, half tiles {old['halves']} -> {new['halves']}, phases {len(new['phases'])}")
    assert new["halves"] <= old["halves"] + 1
    assert np.array_equal(on["status"], off["status"]) and bool(on["status"][0] != 0) == (kind == "foreign"), (on["status"], off["status"])
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"]), (kind, on["ls"], off["ls"])
    assert np.isfinite(on["lg"]).all() and np.isfinite(on["ls"]).all()
    _close(f"{kind}: packed against batch order, dropout on", on["g"], off["g"])
    if kind == "foreign":                                      # the inference forward raises like the reference's nn.Embedding, under both settings
        for p in (True, False):
            with pytest.raises(IndexError):
                _eval(p, x)
    else:
        (lg_on, cnt_on), (lg_off, cnt_off) = _eval(True, x), _eval(False, x)
        assert _bitwise(lg_on, lg_off) and cnt_on == cnt_off and np.isfinite(lg_on).all(), kind
    # dropout-free: both settings at the oracle's grade
    on0, off0 = (_run(p, x, y, w, dropout=False) for p in (True, False))
    assert _bitwise(on0["lg"], off0["lg"]) and _bitwise(on0["ls"], off0["ls"]), kind
    _close(f"{kind}: packed against batch order, dropout-free", on0["g"], off0["g"])
    if kind != "foreign":                                      # (the oracle raises on ids outside the table, as the reference does)
        ref = c["ref"] if kind == "mixed" else G.references(c["sd"], c["fe"], x, y, w, chrom=0)
        for label, r in (("packed", on0), ("batch order", off0)):
            G.assert_grade(f"{kind}: {label}", G.grade(_got(r["lg"], r["ls"], r["g"]), ref))


def test_mixed_batch_reorders_and_saves_tiles():
    """The shared batch is one the order has something to do on: not the identity, fewer half tiles."""
    c = _c23()
    new, old = R.plan(c["x"], 150), R.plan(c["x"], 150, packed=False)
    assert not np.array_equal(new["row_src"], np.arange(len(c["x"]))) and new["halves"] < old["halves"]


@pytest.mark.parametrize("route", ["deterministic", "per_token"])
def test_other_routes(route):
    """`deterministic` (fixed-order sums, per-token front end) and the per-token route (disable_node_front): forward bitwise, gradients within the bound."""
    c = _c23()
    kw = dict(deterministic=True) if route == "deterministic" else dict(node=False)
    on, off = (_run(p, c["x"], c["y"], c["w"], dropout=True, **kw) for p in (True, False))
    assert "node_scatter_kernel" not in on["counts"] and on["counts"] == off["counts"], (on["counts"], off["counts"])
    _plan_equals_twin(f"{route}: packed", c["x"], on, True)
    _plan_equals_twin(f"{route}: batch order", c["x"], off, False)
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"])
    _close(f"{route}: packed against batch order", on["g"], off["g"])
    if route == "deterministic":                                # the packed order is a function of the batch: the fixed-order sums stay reproducible
        again = _run(True, c["x"], c["y"], c["w"], dropout=True, **kw)
        for n, v in on["g"].items():
            assert v is None or np.array_equal(v, again["g"][n]), n


def test_adj_front_end():
    from tests.helpers import oracle_state
    c = _c23()
    _, _, sd = oracle_state(synth.LAYOUTS["c23"], 64, "adj", 72)
    on, off = (_run(p, c["x"], c["y"], c["w"], dropout=True, mode="adj", sd=sd, seed=72, chrom=3) for p in (True, False))
    assert on["counts"] == off["counts"] and "fused_fwd32_kernel" in on["counts"], (on["counts"], off["counts"])
    _plan_equals_twin("adj: packed", c["x"], on, True)
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"])
    _close("adj: packed against batch order", on["g"], off["g"])


def _three_steps(x, y, w, weights=None):
    """Three optimiser steps of the default (packed) setting on a fresh model and Trainer: [(the weights the step ran on, its logits, its losses)].
    ``weights``: the flat parameter buffer to run each step on, copied over in front of it (tests/test_hip_fwd_values.py's form)."""
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=_c23()["sd"])
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    want = R.plan(x, 150)
    seen = []
    for step in range(3):
        if weights is not None:
            tr.rt.flat.copy_(weights[step])
        before = tr.rt.flat.clone()
        with _lib.launch_log() as log:
            tr.step(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("row_fill_kernel", 0) == 1 and log.counts.get("fused_fwd32_kernel", 0) == 1, log.counts
        ws, lg = tr._buffers(*xd.shape)
        assert np.array_equal(_plan(ws, *x.shape)["row_off"].view(np.int32), want["row_off"]) and np.array_equal(_row_src(tr, ws, *x.shape), want["row_src"])
        seen.append((before, lg.cpu().numpy().copy(), tr.losses.cpu().numpy().copy()))
        assert np.isfinite(seen[-1][1]).all() and np.isfinite(seen[-1][2]).all()
    assert all(bool(torch.isfinite(p).all()) for p in clf.parameters())
    return seen


@pytest.mark.parametrize("kind", ["mixed", "pads_and_empty"])
def test_three_optimiser_steps_on_a_poisoned_workspace_equal_a_clean_run(kind, monkeypatch):
    """The packed order keeps row_src, the class counts, the schedule and the plan-order y / w in regions of the plan that older contents may
    occupy: one of them read before it is written shows up as NaN on the poisoned workspace, or as a difference to the clean one -- at the first step
    or, over what the step before left there, at a later one.  The gradients pass through float atomics, so two runs' weights part after the first
    update; the forward has none.  The clean run therefore takes, in front of each step, the weights the poisoned run had there: logits and losses of
    ALL three steps are compared BITWISE."""
    x, y, w = _batch(kind)
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")
    poisoned = _three_steps(x, y, w)
    monkeypatch.delenv("MATCHA_POISON_WS")
    clean = _three_steps(x, y, w, weights=[p[0] for p in poisoned])
    assert not torch.equal(poisoned[0][0], poisoned[1][0]) and not torch.equal(poisoned[1][0], poisoned[2][0])      # the weights did move
    assert not _bitwise(poisoned[0][1], poisoned[1][1]) and not _bitwise(poisoned[1][1], poisoned[2][1])
    for step in range(3):
        assert torch.equal(clean[step][0], poisoned[step][0])
        assert _bitwise(clean[step][1], poisoned[step][1]) and _bitwise(clean[step][2], poisoned[step][2]), (kind, step, clean[step][2], poisoned[step][2])


def test_three_optimiser_steps_and_the_switch_between_steps():
    """Three steps on ONE workspace that starts as NaN, under both settings: the first step's logits and losses bitwise between them, everything
    finite, the weights move.  Then the switch flipped between two steps of one Trainer: each step's plan is its own setting's."""
    from matcha_amd.engine import Trainer
    c = _c23()
    first = {}
    for pack in (True, False):
        clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
        clf.train()
        with _setting(pack):
            tr = Trainer(clf, lr=1e-3, base_seed=11)
            xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
            seen = []
            for i in range(3):
                _, _, lg = tr.step(xd, yd, wd, 1.0, 0.001, 0)
                torch.cuda.synchronize()
                seen.append(lg.cpu().numpy().copy())
                ls = tr.losses.cpu().numpy().copy()
                assert np.isfinite(ls).all() and np.isfinite(seen[-1]).all(), (pack, i, ls)
                assert all(bool(torch.isfinite(p).all()) for p in clf.parameters()), (pack, i)
                if i == 0:
                    first[pack] = (seen[0], ls)
        assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])
    assert _bitwise(first[True][0], first[False][0]) and _bitwise(first[True][1], first[False][1])
    # one Trainer, dropout-free, the same batch: packed, batch order, packed
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    want = {p: R.plan(c["x"], 150, packed=p)["row_off"] for p in (True, False)}
    outs = []
    for pack in (True, False, True):
        with _setting(pack):
            tr.gflat.zero_()
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        ws, _ = tr._buffers(*c["x"].shape)
        assert np.array_equal(_plan(ws, *c["x"].shape)["row_off"].view(np.int32), want[pack]), pack
        outs.append((lg.cpu().numpy().copy(), _grads(tr, clf)))
    assert _bitwise(outs[0][0], outs[1][0]) and _bitwise(outs[0][0], outs[2][0])
    _close("switch flipped: batch order against packed", outs[1][1], outs[0][1])
    _close("switch flipped back", outs[2][1], outs[0][1])


def test_graph_replay_equals_eager():
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    torch.cuda.synchronize()
    g_eager = _grads(tr, clf)
    ws = tr._buffers(*c["x"].shape)[0]
    plan_eager, src_eager = _plan(ws, *c["x"].shape), _row_src(tr, ws, *c["x"].shape)
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
    ws.fill_(0xFF)                                                               # the replay rebuilds the plan, its schedule and row_src from NaN bytes
    graph.replay()
    torch.cuda.synchronize()
    assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
    plan_replay = _plan(ws, *c["x"].shape)
    for n in ("row_off", "count", "tok_key", "half_meta"):
        assert np.array_equal(plan_replay[n], plan_eager[n]), n
    assert np.array_equal(_row_src(tr, ws, *c["x"].shape), src_eager)
    _close("one replay against eager", _grads(tr, clf), g_eager)
