"""The regression task mode (main.py:60-117) on the GPU: the softplus-MSE step of Trainer(objective="regress") on every loss site
(fused embed_dim 64 small and large batch, table and adj front ends; head_fwd / head_bwd at embed_dim 128) against the autograd route
through dlogits, the BCE case of the new entry points against matcha_forward / matcha_backward, the pair records of
matcha_step_record_pairs against their numpy twin, and the driver's regress epochs, CLI and pairwise sweep.  GPU only (-m gpu)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests.test_cpu_regress import pair_permutation, pair_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_dropout(clf):
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0


def _regress_batch(rng, N, ks, rows_per_k):
    """x int64 [B, L]; targets y float32 [B]: alternating rows are positives (a weight in [0.5, 4), some of them repeated so that
    equal-target pairs occur) and negatives (0)."""
    x, _, _ = synth.make_batch(rng, N, ks, rows_per_k)
    B = len(x)
    y = np.zeros(B, dtype=np.float32)
    w = rng.uniform(0.5, 4.0, size=B).astype(np.float32)
    w[::7] = 1.5
    y[0::2] = w[0::2]
    return torch.from_numpy(x), torch.from_numpy(y)


def _trainer_grads(tr, clf):
    rt = tr.rt
    names = {id(p): n for n, p in clf.named_parameters()}
    touched = tr.touched.cpu().tolist()
    out = {n: None for n, _ in clf.named_parameters()}
    for p, o, grp in zip(rt.live, rt.seg_off_list[:-1], rt.seg_group_list):
        if touched[grp]:
            out[names[id(p)]] = tr.gflat[o:o + p.numel()].view(p.shape).clone()
    return out


# name -> (layout, embed_dim, front end, ks, rows per k, kernels that must run with loss_in_forward on)
CASES = {
    "tiny_table_d64": ("tiny", 64, "table", [2, 3, 5], 20, {"fused_fwd32h_kernel"}),
    "tiny_adj_d64": ("tiny", 64, "adj", [2, 3, 5], 20, {"fused_fwd32h_kernel"}),
    "hg38_table_d64": ("hg38_1mb", 64, "table", [2, 3, 4, 5], 2304, {"fused_fwd32_kernel", "tail_bwd64_kernel"}),
    "hg38_adj_d64": ("hg38_1mb", 64, "adj", [2, 3, 4, 5], 2304, {"fused_fwd32_kernel", "tail_bwd64_kernel", "adj_fused_fwd_kernel"}),
    "c1_table_d128": ("c1", 128, "table", [2, 3, 4, 5], 1024, {"enc128_fwd_kernel", "head_fwd_kernel", "head_bwd_kernel"}),
}


def _assert_kernels(name, lif, ran):
    """The path of each case: with the tail's backward in the forward kernel (lif) the table's kernels; without it the same forward kernel
    and the tail's backward as head_bwd_kernel (never tail_bwd64_kernel)."""
    must = set(CASES[name][5])
    must_not = set()
    if not lif and CASES[name][1] == 64:
        must = (must - {"tail_bwd64_kernel"}) | {"head_bwd_kernel"}
        must_not = {"tail_bwd64_kernel"}
    assert must <= ran, (name, lif, sorted(must - ran), sorted(ran))
    assert not (must_not & ran), (name, lif, sorted(must_not & ran))


@pytest.mark.parametrize("lif", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_regress_step_matches_the_autograd_route(name, lif):
    """One dropout-free step, alpha = 1 / beta = 1e-3: Trainer(objective="regress") -- the loss and its logit gradient inside the
    kernels -- against model(x) -> F.softplus -> F.mse_loss (+ beta * recon) -> backward (the unfused backward through dlogits):
    logits, MSE, recon, the grad-None set and every gradient element; then one AdamW step moves the weights."""
    from matcha_amd.engine import Trainer
    from tests.test_hip_model import hip_model
    layout, d, mode, ks, rows, must = CASES[name]
    num = synth.LAYOUTS[layout]
    clf, _ = hip_model(num, d, mode, 91)
    _no_dropout(clf)
    clf.train()
    x, y = _regress_batch(np.random.default_rng(5), int(np.sum(num)), ks, rows)
    x, y = x.cuda(), y.cuda()
    alpha, beta = 1.0, 1e-3
    # the autograd route (the reconstruction chromosome drawn as Classifier.forward draws it)
    np.random.seed(17)
    chrom = int(np.random.choice(np.arange(len(num)), 1)[0])
    np.random.seed(17)
    lg_ref, rc_ref = clf(x, return_recon=True)
    mse_ref = torch.nn.functional.mse_loss(torch.nn.functional.softplus(lg_ref.view(-1)), y)
    (mse_ref * alpha + rc_ref * beta).sum().backward()
    g_ref = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in clf.named_parameters()}
    for p in clf.parameters():
        p.grad = None
    tr = Trainer(clf, lr=1e-3, objective="regress")
    tr.loss_in_forward = lif
    with _lib.launch_log() as log:
        logits = tr.forward_backward(x, y, None, alpha, beta, chrom)
        torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    _assert_kernels(name, lif, ran)
    e_lg = float((logits - lg_ref.view(-1)).abs().max() / lg_ref.abs().max().clamp_min(1e-3))
    assert e_lg <= 1e-6, e_lg
    assert abs(float(tr.losses[0]) - float(mse_ref)) <= 1e-6 * max(1.0, float(mse_ref)), (float(tr.losses[0]), float(mse_ref))
    assert abs(float(tr.losses[1]) - float(rc_ref.view(-1)[0])) <= 1e-6 * max(1.0, abs(float(rc_ref.view(-1)[0])))
    grads = _trainer_grads(tr, clf)
    none_got = {n for n, v in grads.items() if v is None} - {"attribute_dict_embedding.weight"}
    none_ref = {n for n, v in g_ref.items() if v is None} - {"attribute_dict_embedding.weight"}
    assert none_got == none_ref
    worst, checked = 0.0, 0
    for n, v in grads.items():
        if v is None or g_ref[n] is None:
            continue
        ref = g_ref[n]
        e = float((v - ref).abs().max()) / max(float(ref.abs().max()), 1e-3)
        worst = max(worst, e)
        assert e <= 1e-6, (n, e)             # (measured: at most 7.8e-7 over every case)
        checked += 1
    assert checked >= 20
    before = clf.layer_norm1.weight.detach().clone()
    tr.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(before, clf.layer_norm1.weight.detach())
    print(f"regress {name} lif={lif}: logits {e_lg:.1e}, worst gradient {worst:.1e}; kernels {sorted(ran)}")


def _raw_step(tr, fwd, bwd, x, y, w, alpha, beta, obj=None):
    """Trainer.forward_backward with the C entry points given (same options, same workspace)."""
    rt = tr.rt
    B, L = x.shape
    ws, logits = tr._buffers(B, L)
    opts = tr._opts(alpha, beta, 0)
    st = rt.stream()
    pre = [] if obj is None else [obj]
    _lib.check(fwd(*pre, C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L, _lib.ptr(y), _lib.ptr(w),
                   _lib.ptr(logits), _lib.ptr(tr.losses), _lib.ptr(ws), ws.numel(), st), "forward")
    _lib.check(bwd(*pre, C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L, _lib.ptr(y), _lib.ptr(w), None,
                   None, C.byref(tr.grads), _lib.ptr(tr.touched), _lib.ptr(ws), ws.numel(), st), "backward")
    torch.cuda.synchronize()
    return logits.clone(), tr.losses.clone(), tr.gflat.clone()


def test_bce_objective_is_bitwise_matcha_forward_backward_at_the_bench_shape():
    """objective = BCE through the new entry points computes exactly what matcha_forward / matcha_backward compute (hg38 1 Mb, table,
    embed_dim 64, 65 536 rows; the deterministic table gradient so that two runs can be compared bit for bit)."""
    from matcha_amd.engine import Trainer
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    clf, _ = hip_model(num, 64, "table", 92)
    _no_dropout(clf)
    clf.train()
    x, y, w = synth.make_batch(np.random.default_rng(8), int(np.sum(num)), [2, 3, 4, 5, 6, 7, 8], 65536 // 7 + 1)
    x, y, w = (torch.from_numpy(a[:65536]).cuda().contiguous() for a in (x, y.reshape(-1), w.reshape(-1)))
    tr = Trainer(clf, lr=1e-3, deterministic=True)
    lib = tr.lib
    tr.gflat.zero_()
    a = _raw_step(tr, lib.matcha_forward, lib.matcha_backward, x, y, w, 1.0, 0.001)
    tr.gflat.zero_()
    b = _raw_step(tr, lib.matcha_forward_objective, lib.matcha_backward_objective, x, y, w, 1.0, 0.001, obj=_lib.OBJECTIVE_BCE)
    for u, v, what in zip(a, b, ("logits", "losses", "gradient")):
        assert torch.equal(u, v), what


def _record_pairs(logits, losses, y, x, it, n_steps, seed, sums, preds, labels, sizes):
    B, L = x.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().matcha_step_record_pairs(_lib.ptr(logits), _lib.ptr(losses), _lib.ptr(y), _lib.ptr(x), B, L, _lib.ptr(it), n_steps,
                                                   _lib.ptr(seed), _lib.ptr(sums), _lib.ptr(preds), _lib.ptr(labels), _lib.ptr(sizes), st),
               "matcha_step_record_pairs")


@pytest.mark.parametrize("B", [2, 3, 192, 5000])
def test_step_record_pairs_equals_the_host_twin(B):
    rng = np.random.default_rng(B)
    n_steps, L = 4, 5
    logits = rng.normal(0, 6, size=B).astype(np.float32)
    logits[::5] += 30.0                                      # past softplus' threshold
    y = np.where(rng.random(B) < 0.5, np.round(rng.uniform(0.5, 3.0, size=B), 1), 0.0).astype(np.float32)
    x = np.zeros((B, L), dtype=np.int64)
    k = rng.integers(2, L + 1, size=B)
    for b in range(B):
        x[b, :k[b]] = np.sort(rng.choice(np.arange(1, 1000), k[b], replace=False))
    seed = 0x1234_5678_9ABC
    H = B // 2
    dev = "cuda"
    t = {n: torch.from_numpy(v).to(dev) for n, v in dict(logits=logits, y=y, x=x).items()}
    losses = torch.tensor([0.25, 0.5, 0.0], device=dev)
    it, sums = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(2, device=dev)
    sd = torch.tensor([seed], dtype=torch.long, device=dev)
    preds = torch.full((n_steps, H), -5.0, device=dev)
    labels = torch.full((n_steps, H), -7, dtype=torch.int32, device=dev)
    sizes = torch.full((n_steps, H), -1, dtype=torch.long, device=dev)
    for _ in range(n_steps + 1):                             # one call past the end: overwrites the last row, never out of bounds
        _record_pairs(t["logits"], losses, t["y"], t["x"], it, n_steps, sd, sums, preds, labels, sizes)
    torch.cuda.synchronize()
    assert int(it) == n_steps + 1
    assert torch.allclose(sums.cpu(), torch.tensor([0.25, 0.5]) * (n_steps + 1))
    for s in range(n_steps):
        step = s if s < n_steps - 1 else n_steps     # the last row holds the step past the end
        p_ref, l_ref, s_ref = pair_records(logits, y, x, seed, step)
        pi = pair_permutation(B, seed, step)
        used = pi[:2 * H]
        assert len(np.unique(used)) == len(used)             # every row at most once per step
        assert np.array_equal(labels[s].cpu().numpy(), l_ref), s
        assert np.array_equal(sizes[s].cpu().numpy(), s_ref), s
        assert float(np.abs(preds[s].cpu().numpy() - p_ref).max()) <= 1e-6, s


def test_pair_categories_over_200_steps_are_hypergeometric():
    """A 192-row regress step (96 positives with distinct targets, 96 negatives): over 200 steps the numbers of neg-neg and pos-pos pairs
    fall within 4 sigma of their expectation under a uniformly random perfect matching (pos-neg is the rest)."""
    B, P, n_steps = 192, 96, 200
    H = B // 2
    dev = "cuda"
    y = torch.zeros(B, device=dev)
    y[:P] = torch.linspace(0.5, 4.0, P, device=dev)
    logits = torch.full((B,), -5.0, device=dev)
    logits[:P] = 5.0                 # pred ~ 0.5 for pos-pos and neg-neg pairs, ~ sigmoid(+-5) for mixed pairs
    x = torch.ones((B, 2), dtype=torch.long, device=dev)
    it, sums, sd = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(2, device=dev), torch.tensor([77], dtype=torch.long, device=dev)
    losses = torch.zeros(3, device=dev)
    preds = torch.empty((n_steps, H), device=dev)
    labels = torch.empty((n_steps, H), dtype=torch.int32, device=dev)
    sizes = torch.empty((n_steps, H), dtype=torch.long, device=dev)
    for _ in range(n_steps):
        _record_pairs(logits, losses, y, x, it, n_steps, sd, sums, preds, labels, sizes)
    torch.cuda.synchronize()
    lab, pr = labels.cpu(), preds.cpu()
    nn = int((lab == -1).sum())
    pp = int(((lab >= 0) & ((pr - 0.5).abs() < 0.01)).sum())
    pn = n_steps * H - nn - pp
    # one step: X = number of pairs with both rows among the 96 of one class; P(pair both) = p, P(two given pairs both) = q
    p = (P * (P - 1)) / (B * (B - 1))
    q = (P * (P - 1) * (P - 2) * (P - 3)) / (B * (B - 1) * (B - 2) * (B - 3))
    mean = H * p
    var = H * p * (1 - p) + H * (H - 1) * (q - p * p)
    sig = np.sqrt(n_steps * var)
    assert abs(nn - n_steps * mean) <= 4 * sig, (nn, n_steps * mean, sig)
    assert abs(pp - n_steps * mean) <= 4 * sig, (pp, n_steps * mean, sig)
    assert pn == n_steps * H - nn - pp and pn > 0


def _epoch_setup(layout, d, mode, seed):
    from matcha_amd import train as T
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(3)
    edges = np.concatenate([np.pad(synth.make_edges(rng, N, k, 400), ((0, 0), (0, 3 - k))) for k in (2, 3)])
    weights = (rng.uniform(0.2, 1.0, size=len(edges)) * 3).astype(np.float32)
    np.random.seed(5)
    torch.manual_seed(5)
    clf, _ = hip_model(num, d, mode, seed)
    clf.train()
    sess = T.Session(clf, synth.node2chrom(num), synth.chrom_range(num).astype(np.int32), 2, 3, 0, seed=11, deterministic=True,
                     task_mode="regress")
    sess.set_known(edges)
    return T, sess, edges, weights


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_regress_epoch_graph_replay_equals_the_step_function(mode, monkeypatch):
    """train_epoch / eval_epoch with task_mode 'regress': the captured step replayed per batch (one replay per step) reports what the same
    device-side step function enqueued call by call (MATCHA_TRAIN_GRAPH=steps) reports -- loss sums and metric strings -- and the training
    epochs equal the torch-assembled call-by-call loop (a new batch of positives every step)."""
    from matcha_amd import train as T0
    res = {}
    for how in ("steps", "graph", "eager"):
        if how == "steps":
            monkeypatch.setenv("MATCHA_TRAIN_GRAPH", "steps")
        else:
            monkeypatch.delenv("MATCHA_TRAIN_GRAPH", raising=False)
        T0.GRAPH_EPOCHS = how != "eager"
        try:
            T, sess, edges, weights = _epoch_setup("c23", 64, mode, 81)
            assert sess.neg_num == 1 and sess.graph_ok(0.001) == (how != "eager")
            r0 = T.STATS["train_graph_replays"]
            out = [T.train_epoch(sess, edges, weights, 1.0, 0.001, batch_size=24) for _ in range(2)]
            n_batch = len(edges) // 24
            replays = T.STATS["train_graph_replays"] - r0
            torch.cuda.synchronize()
        finally:
            T0.GRAPH_EPOCHS = True
        if how == "eager":
            res[how] = (out, replays, n_batch)
            continue
        out.append(T.eval_epoch(sess, edges, weights, batch_size=24))
        torch.cuda.synchronize()
        res[how] = (out, replays, n_batch)
    (o0, r_steps, n_batch), (o1, r_graph, _) = res["steps"], res["graph"]
    assert r_steps == 0
    assert r_graph == 2 * n_batch - 2                      # the first two steps of the first epoch run eagerly before the capture
    for a, b in zip(o0, o1):
        assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(a[0])), (a, b)
        assert abs(a[1] - b[1]) <= 1e-3 * max(1.0, abs(a[1])), (a, b)
        if mode == "table":
            assert a[2:] == b[2:], (a, b)
    for a, b in zip(res["eager"][0], o1[:2]):
        assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(a[0])), (a, b)
        assert abs(a[1] - b[1]) <= 1e-3 * max(1.0, abs(a[1])), (a, b)
        if mode == "table":
            assert a[2:] == b[2:], (a, b)


def test_regress_call_by_call_epoch_and_falling_mse():
    """The call-by-call branches (no graph) run the same objective and pair records; on synthetic data the training MSE falls.  (The
    synthetic weights do not depend on the nodes, so the MSE can only approach the targets' spread: ~1.05 when the model predicts
    their mean, ~0.24 when it separates positives from negatives perfectly; six short epochs move it ~12 % from its start.)"""
    from matcha_amd import train as T0
    T0.GRAPH_EPOCHS = False
    try:
        T, sess, edges, weights = _epoch_setup("tiny", 16, "table", 83)
        assert not sess.graph_ok(1.0)
        mses = [T.train_epoch(sess, edges, weights, 1.0, 0.0, batch_size=48)[0] for _ in range(6)]
        ev = T.eval_epoch(sess, edges, weights, batch_size=48)
    finally:
        T0.GRAPH_EPOCHS = True
    assert all(np.isfinite(mses)) and np.isfinite(ev[0])
    assert mses[-1] < 0.95 * mses[0], mses
    T1, sess1, _, _ = _epoch_setup("tiny", 16, "table", 83)
    mses_g = [T1.train_epoch(sess1, edges, weights, 1.0, 0.0, batch_size=48)[0] for _ in range(6)]
    assert mses_g[-1] < 0.95 * mses_g[0], mses_g


def test_train_cli_regress_writes_the_reference_outputs(tmp_path):
    from tests.test_train_driver import _write_temp_dir
    cfg, num = _write_temp_dir(str(tmp_path), m=600)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "matcha_amd.train", "--config", os.path.join(str(tmp_path), "config.JSON"), "--front-end", "table",
                        "--task-mode", "regress", "--epochs1", "1", "--epochs2", "1", "--batches-per-epoch", "2"],
                       cwd=os.path.join(str(tmp_path), "Temp"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    temp = cfg["temp_dir"]
    assert os.path.exists(os.path.join(temp, "model.chkpt")) and os.path.exists(os.path.join(temp, "model2load"))
    emb = np.load(os.path.join(str(tmp_path), "embeddings.npy"))
    assert emb.shape == (int(np.sum(num)), 16) and np.isfinite(emb).all()
    assert "Training" in r.stdout


def test_pairwise_sweep_regress_is_softplus_of_the_logits():
    from matcha_amd import predict as PR
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["tiny"]
    clf, _ = hip_model(num, 16, "table", 93)
    cr = synth.chrom_range(num)
    pairs, p_cls = PR.pairwise_probabilities(clf, cr, 0, 0)
    pairs_r, p_reg = PR.pairwise_probabilities(clf, cr, 0, 0, task_mode="regress")
    assert torch.equal(pairs, pairs_r)
    with torch.no_grad():
        lg = clf(pairs.contiguous()).reshape(-1)
    assert torch.allclose(p_reg, torch.nn.functional.softplus(lg), rtol=0, atol=1e-6)
    assert torch.allclose(p_cls, torch.sigmoid(lg), rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        PR.pairwise_probabilities(clf, cr, 0, 0, task_mode="rank")


_DP_SCRIPT = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, {root!r})
import torch.distributed as dist
from matcha_amd import synth
from matcha_amd.engine import Trainer
from tests.test_hip_model import hip_model
from tests.test_hip_regress import _regress_batch, _no_dropout
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
num = synth.LAYOUTS["c23"]
clf, _ = hip_model(num, 64, "table", 94)
_no_dropout(clf); clf.train()
x, y = _regress_batch(np.random.default_rng(9), int(np.sum(num)), [2, 3, 4], 256)
x, y = x.cuda(), y.cuda()
tr = Trainer(clf, lr=1e-3, objective="regress", table_exchange="dense")
B = len(x) // world
tr.forward_backward(x[rank * B:(rank + 1) * B].contiguous(), y[rank * B:(rank + 1) * B].contiguous(), None, 1.0, 0.001)
tr.all_reduce()
torch.cuda.synchronize()
if rank == 0:
    np.save({out!r}, (tr.gflat / world).cpu().numpy())
dist.destroy_process_group()
"""


def test_two_ranks_regress_step_equals_the_single_rank_global_batch(tmp_path):
    """Data parallel (two ranks sharing the GPU over gloo, the test_hip_data_parallel.py pattern): each rank steps on half of the batch;
    the MSE is a mean over rows like the BCE, so the all-reduced gradient scaled by 1/world (what AdamW applies) equals the single-rank
    gradient of the whole batch."""
    from matcha_amd.engine import Trainer
    from tests.test_hip_model import hip_model
    out = os.path.join(str(tmp_path), "dp.npy")
    script = os.path.join(str(tmp_path), "dp.py")
    with open(script, "w") as f:
        f.write(_DP_SCRIPT.format(root=ROOT, out=out))
    from tests.test_hip_data_parallel import _free_port
    port = _free_port()
    procs = []
    try:
        for rank in range(2):
            env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PYTHONPATH=ROOT)
            procs.append(subprocess.Popen([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        for p in procs:
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, err[-3000:]
    finally:
        for p in procs:                      # a time-out or a failed rank: no child is left holding the GPU
            if p.poll() is None:
                p.kill()
                p.wait()
    num = synth.LAYOUTS["c23"]
    clf, _ = hip_model(num, 64, "table", 94)
    _no_dropout(clf)
    clf.train()
    x, y = _regress_batch(np.random.default_rng(9), int(np.sum(num)), [2, 3, 4], 256)
    tr = Trainer(clf, lr=1e-3, objective="regress")
    tr.forward_backward(x.cuda(), y.cuda(), None, 1.0, 0.001)
    torch.cuda.synchronize()
    single = tr.gflat.cpu().numpy()
    dp = np.load(out)
    assert dp.shape == single.shape
    for o0, o1 in zip(tr.rt.seg_off_list[:-1], tr.rt.seg_off_list[1:]):       # tensor by tensor, relative to each one's largest element
        ref, got = single[o0:o1], dp[o0:o1]
        assert float(np.abs(got - ref).max()) <= 1e-5 * float(np.abs(ref).max()) + 2e-8, o0


# ---- the gr_* fixtures of the REAL reference (tests/golden/make_golden_regress.py) ------------------------------------------------------
TOL = 1e-4
GR_KERNELS = {"tiny_table": "tiny_table_d64", "tiny_adj": "tiny_adj_d64", "hg38_table_d64": "hg38_table_d64", "hg38_adj_d64": "hg38_adj_d64",
              "c1_table_d128": "c1_table_d128"}


@pytest.mark.parametrize("lif", [True, False])
@pytest.mark.parametrize("name", sorted(GR_KERNELS))
def test_regress_steps_match_the_reference_fixture(name, lif):
    """Trainer(objective="regress") on the reference's own regress steps (forward_op_batch_regress with y given, AdamW): logits, MSE,
    recon, the grad-None set and every stored gradient element of step 0 at TOL, the parameters after the first and the last step, and
    the kernel set of the case's path."""
    from matcha_amd.engine import Trainer
    from tests.helpers import gold, logit_err
    from tests.test_cpu_regress import GR, GAUGE, gr_ref, gr_n_steps
    from tests.test_hip_model import hip_model
    layout, d, mode, seed = GR[name]
    g = gold(f"gr_{name}.npz")
    clf, _ = hip_model(synth.LAYOUTS[layout], d, mode, seed)
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, objective="regress")
    tr.loss_in_forward = lif
    n_steps = gr_n_steps(g)
    n_param = 0
    for step in range(n_steps):
        x = torch.from_numpy(g[f"x{step}"].astype(np.int64)).cuda()
        y = torch.from_numpy(g[f"y{step}"]).reshape(-1).cuda()
        with _lib.launch_log() as log:
            logits = tr.forward_backward(x, y, None, float(g["alpha"][step]), float(g["beta"][step]), int(g["chroms"][step]))
            torch.cuda.synchronize()
        if step == 0:
            _assert_kernels(GR_KERNELS[name], lif, {k for k, n in log.counts.items() if n > 0})
        assert logit_err(logits.cpu().numpy(), g[f"logits{step}"].reshape(-1)) < (TOL if step == 0 else 2 * TOL), step
        assert abs(float(tr.losses[0]) - float(g[f"mse{step}"])) < TOL * max(1.0, float(g[f"mse{step}"])), step
        assert abs(float(tr.losses[1]) - float(g[f"recon{step}"][0])) < TOL * max(1.0, abs(float(g[f"recon{step}"][0]))), step
        if step == 0:
            grads = _trainer_grads(tr, clf)
            assert {n for n, v in grads.items() if v is None} - {"attribute_dict_embedding.weight"} == \
                set(g["grad_none"].tolist()) - {"attribute_dict_embedding.weight"}
            checked = 0
            for n, v in grads.items():
                if v is None or n == GAUGE:
                    continue
                stride, ref = gr_ref(g, "grad0", n)
                got = v.cpu().numpy().reshape(-1)[::stride]
                assert np.abs(got - ref).max() <= TOL * max(np.abs(ref).max(), 1e-3), n
                checked += 1
            assert checked >= 20
        tr.optimizer_step()
        if step in (0, n_steps - 1):
            torch.cuda.synchronize()
            for n, p in clf.named_parameters():
                stride, ref = gr_ref(g, f"param{step}", n)
                if stride is None or n == GAUGE:
                    continue
                diff = np.abs(p.detach().cpu().numpy().reshape(-1)[::stride] - ref)
                scale = max(np.abs(ref).max(), 1e-3)
                # AdamW's first steps are lr * sign(g) where |g| is near eps: rounding noise of a near-zero gradient (the reference's too)
                # can flip one element's step; the bulk agrees to 2 TOL of the tensor's scale (tests/test_hip_model.py::_train_g3)
                assert np.quantile(diff, 0.999) <= 2 * TOL * scale, (step, n)
                assert diff.max() <= 2.05e-3 * (step + 1), (step, n)
                n_param += 1
    assert n_param >= 40
