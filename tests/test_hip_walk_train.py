"""The walk initialisation through the public surface: matcha_amd.train.run(table_init=...) on synthetic data and the two
files of ``python -m matcha_amd.walk``.  GPU only (-m gpu)."""
import os

import numpy as np
import pytest
import torch

from matcha_amd import walk as Wk
from tests.test_train_driver import _write_temp_dir

pytestmark = pytest.mark.gpu


def _run(tmp_path, monkeypatch, **kw):
    """One short train.run at d = 64; returns (config, N, the table as the first training epoch found it, the log lines)."""
    from matcha_amd import train as T
    import Modules  # noqa: F401
    cfg, num = _write_temp_dir(str(tmp_path), m=600, d=64)
    seen = {}
    real_train = T.train

    def spy(sess, *a, **k):
        seen.setdefault("table", sess.model.node_embedding.weight.detach().clone())
        return real_train(sess, *a, **k)
    monkeypatch.setattr(T, "train", spy)
    np.random.seed(0)
    torch.manual_seed(0)
    logs = []
    T.run(cfg, front_end="table", epochs1=1, epochs2=1, batches_per_epoch=2, emb_path=os.path.join(tmp_path, "emb.npy"), log=logs.append, **kw)
    return cfg, int(np.sum(num)), seen["table"], logs


def test_train_run_starts_from_the_walk_embeddings(tmp_path, monkeypatch):
    from matcha_amd import train as T
    made = {}
    real = Wk.walk_embeddings

    def spy(edges, n_nodes, d, **kw):
        made["args"] = (edges.clone(), n_nodes, d, kw)
        made["out"] = real(edges, n_nodes, d, **kw)
        return made["out"].clone()
    monkeypatch.setattr(Wk, "walk_embeddings", spy)
    opts = dict(num_walks=4, walk_length=12, window=3, p=2.0, q=0.25)
    cfg, N, table, logs = _run(tmp_path, monkeypatch, table_init="walk", walk_opts=opts)
    edges, n_nodes, d, kw = made["args"]
    data, _ = T.load_kmers(cfg["temp_dir"], [2, 3], 0.6)
    seed = kw.pop("seed")                                        # drawn from numpy's generator where the caller names none
    assert (n_nodes, d, kw) == (N, 64, opts) and 0 <= seed < 1 << 31
    assert np.array_equal(edges.cpu().numpy(), data)             # the positives, as the reference passes them
    assert torch.equal(table, made["out"]) and table.shape == (N + 1, 64) and (table[0] == 0).all()
    body = table[1:].double()
    assert float(body.mean(0).abs().max()) < 1e-5 and float((body.pow(2).mean(0).sqrt() - 1).abs().max()) < 1e-5
    assert any("Training" in l for l in logs) and all(np.isfinite(float(l.split("bce:")[1].split(",")[0])) for l in logs if "Training" in l)


def test_random_init_computes_what_the_commit_before_the_feature_computed(tmp_path):
    """table_init="random", named or left to the default, against tests/golden/walk_parent_random_init.npz -- what tests/walk_init_probe.py
    recorded on the commit before this feature, on an MI355X: the table, the eval-mode logits of the freshly initialised model (every
    parameter enters them), the states of torch's CPU and device generators and of numpy's generator once the model is built, and the
    logits after the run's training steps (deterministic table gradient) -- all bit for bit."""
    from tests.helpers import GOLD
    from tests.walk_init_probe import probe
    gold = np.load(os.path.join(GOLD, "walk_parent_random_init.npz"))
    assert all(bool(r) for r in gold["repeatable"]), dict(zip(gold["keys"].tolist(), gold["repeatable"].tolist()))   # the parent agreed with itself
    for i, kw in enumerate(({"table_init": "random"}, {})):
        (tmp_path / str(i)).mkdir()
        got = probe(tmp_path / str(i), **kw)
        assert sorted(got) == gold["keys"].tolist()
        for k in got:
            assert np.array_equal(got[k], gold[k]), (kw, k)


def test_table_from_a_file_and_refusals(tmp_path, monkeypatch):
    """A .npy of unscaled vectors is scaled into the table like the walk's; the adj front end has no table to initialise."""
    cfg, N, _, _ = _run(tmp_path, monkeypatch, table_init="random")
    A = np.random.default_rng(2).normal(size=(N, 64)).astype(np.float32) * 3 + 1
    np.save(tmp_path / "wv.npy", A)
    monkeypatch.undo()
    (tmp_path / "b").mkdir()
    cfg, N, table, _ = _run(tmp_path / "b", monkeypatch, table_init=str(tmp_path / "wv.npy"))
    assert (table[0] == 0).all() and torch.equal(table[1:].cpu(), Wk.standard_scale(torch.from_numpy(A)))
    from matcha_amd import train as T
    np.save(tmp_path / "bad.npy", A[:, :32])
    with pytest.raises(ValueError, match="the table needs"):
        T.run(cfg, front_end="table", table_init=str(tmp_path / "bad.npy"), emb_path=None, log=lambda *_: None)
    with pytest.raises(ValueError, match="table front end"):
        T.run(cfg, front_end="adj", table_init="walk")


def test_cli_writes_the_references_two_files(tmp_path):
    from matcha_amd import train as T
    cfg, num = _write_temp_dir(str(tmp_path), m=600, d=64)
    N = int(np.sum(num))
    out, txt = str(tmp_path / "tiny_wv_64_hyper.npy"), str(tmp_path / "walks.txt")
    Wk.main(["--config", str(tmp_path / "config.JSON"), "-o", out, "--save-walks", txt, "--num-walks", "2", "--walk-length", "6", "--seed", "4"])
    wv = np.load(out)
    assert wv.shape == (N, 64) and wv.dtype == np.float32 and np.isfinite(wv).all() and np.abs(wv).max() > 0.5 / 64
    lines = open(txt).read().splitlines()
    assert len(lines) == 2 * N and all(len(l.split(" ")) == 6 for l in lines)                 # np.savetxt(fmt="%d", delimiter=" ")
    walks = np.loadtxt(txt, delimiter=" ").astype(np.int64)
    data, _ = T.load_kmers(cfg["temp_dir"], [2, 3], 0.6)
    graph = Wk.HyperWalkGraph(torch.from_numpy(np.ascontiguousarray(data).astype(np.int64)).cuda(), N)
    again, _ = Wk.hyper_walks(graph, 2, 6, seed=4)
    assert np.array_equal(walks, again.cpu().numpy().astype(np.int64) - 1) and walks.min() >= 0 and walks.max() <= N - 1      # 0-based ids
