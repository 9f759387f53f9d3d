"""Fine-tune a loaded model on hyperedges of any width 2 .. 32: the reference's step (forward_op_batch, main.py:37-58) call by call.

    python -m matcha_amd.finetune --config ./config.JSON --model model2load --sizes 9 12 --epochs N -o OUT

reads temp_dir/all_<k>_counter.npy / all_<k>_freq_counter.npy for the sizes given (train.load_kmers), splits them 80 / 20, trains on
positives and device-sampled negatives with torch.optim.AdamW and saves the model the way train.py does (a state-dict checkpoint and a
pickled ``model2load``).

A step is generate_negative (main.py:361-459) -> model -> alpha * weighted BCE + beta * reconstruction -> backward -> AdamW.  Rows of
9 to 32 columns go through the model's long training pair (Classifier.long_row_training: matcha_forward_long_train /
matcha_backward_long) and the long sampler (matcha_neg_sample_long); rows of up to 8 columns through the ordinary autograd path and
matcha_neg_sample.  The fused engine.Trainer, the captured (hipGraph) epochs, the data-parallel path and train.py stay at 8 columns:
this loop is eager, single GPU, and synchronises once per epoch.
"""
from __future__ import annotations

import argparse
import os
import time
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import utils as U
from .sampler import HyperedgeSet, NegativeSampler

BATCH_SIZE = 96          # main.py:527
NEG_NUM = 3              # main.py:528


class LongRowSession:
    """Model, known-hyperedge set, negative sampler and AdamW for rows of up to 32 columns.

    ``known_edges``: int64 [M, L <= 32] zero-padded ascending rows (numpy or tensor; None or empty = the reference's phase 1, where
    negatives equal their positives); ``node2chrom`` int32 [N + 1], ``chrom_range`` int32 [C, 2] as train.Session takes them."""

    regress = False          # train._metrics reads it: the class objective only

    def __init__(self, model, known_edges, node2chrom: np.ndarray, chrom_range: np.ndarray, neg_num: int = NEG_NUM, min_dis: int = 0,
                 lr: float = 1e-3, seed: int = 0):
        self.model = model
        self.dev = model.layer_norm1.weight.device
        model.long_row_training = True
        self.neg_num, self.min_dis = int(neg_num), int(min_dis)
        if known_edges is None or len(known_edges) == 0:
            width = _lib.MAX_LONG_L if known_edges is None else int(np.shape(known_edges)[1])
            self.hset = HyperedgeSet.empty(self.dev, width)
        else:
            self.hset = HyperedgeSet(torch.as_tensor(np.ascontiguousarray(known_edges) if isinstance(known_edges, np.ndarray) else known_edges)
                                     .to(self.dev))
        self.max_size = self.hset.L
        self.sampler = NegativeSampler(self.hset, node2chrom, chrom_range, neg_num=self.neg_num, min_dis=self.min_dis, seed=seed)
        self.opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=lr)      # main.py:630

    def check_status(self) -> int:
        """Synchronising read of the device status words: IndexError for a node id outside [0, N] (the model's), KeyError for a node without
        a chromosome (the sampler's); returns the number of negatives whose 65 536 redraws were exhausted since the last call."""
        self.model.check_status()
        return self.sampler.check_status()

    def make_batch(self, pos: torch.Tensor, pos_w: torch.Tensor):
        """generate_negative's output (main.py:443-448), like train.Session.make_batch: x = [pos; neg] with the negatives of positive j
        at rows P + neg_num*j ..., y = [1..; 0..], w = [pos_w..; 1..], sizes = non-zero entries per row."""
        pos = pos.to(device=self.dev, dtype=torch.long).contiguous()
        P = pos.shape[0]
        neg = self.sampler.sample(pos)
        x = torch.cat([pos, neg], dim=0)
        y = torch.cat([torch.ones(P, device=self.dev), torch.zeros(neg.shape[0], device=self.dev)])
        w = torch.cat([pos_w.to(device=self.dev, dtype=torch.float32).reshape(-1), torch.ones(neg.shape[0], device=self.dev)])
        return x, y, w, (x != 0).sum(dim=1)

    def _loss(self, x, y, w, alpha: float, beta: float):
        m = self.model
        had, prev = "check_ids" in m.__dict__, m.check_ids
        m.__dict__["check_ids"] = False                  # no status read-back per forward: check_status() reads it once
        try:
            logits, recon = m(x, return_recon=True)
        finally:
            if had:
                m.__dict__["check_ids"] = prev
            else:
                m.__dict__.pop("check_ids", None)
        logits = logits.view(-1)
        bce = F.binary_cross_entropy_with_logits(logits, y, weight=w)
        recon = recon.reshape(-1)[0]
        return alpha * bce + beta * recon, bce, recon, logits

    def step(self, pos: torch.Tensor, pos_w: torch.Tensor, alpha: float = 1.0, beta: float = 0.001):
        """One training step on ``pos`` int64 [P, L] / ``pos_w`` float32 [P]: returns (bce, recon, logits [B], y [B], sizes [B]) as
        device tensors, B = P * (1 + neg_num).  Nothing synchronises: node ids and chromosomes are checked on the device and read with
        check_status()."""
        self.model.train()
        x, y, w, sizes = self.make_batch(pos, pos_w)
        self.last_batch = (x, y, w, sizes)
        loss, bce, recon, logits = self._loss(x, y, w, alpha, beta)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return bce.detach(), recon.detach(), logits.detach(), y, sizes

    def _epoch(self, edges, weights, batch_size, alpha, beta, training: bool, max_rows: Optional[int]):
        from .train import _metrics
        e = torch.as_tensor(edges).to(self.dev)
        w = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(self.dev)
        perm = torch.from_numpy(np.random.permutation(len(e))[:max_rows]).to(self.dev)      # sync_shuffle, utils.py:142-149
        e, w = e[perm], w[perm]
        n_batch = len(e) // batch_size
        bce_sum, rec_sum = torch.zeros((), device=self.dev), torch.zeros((), device=self.dev)
        preds, labels, sizes = [], [], []
        for i in range(n_batch):                         # nothing synchronises inside the loop
            pos, pw = e[i * batch_size:(i + 1) * batch_size], w[i * batch_size:(i + 1) * batch_size]
            if training:
                bce, recon, logits, y, s = self.step(pos, pw, alpha, beta)
            else:
                x, y, ww, s = self.make_batch(pos, pw)
                _, bce, recon, logits = self._loss(x, y, ww, alpha, beta)
            bce_sum += bce
            rec_sum += recon
            preds.append(torch.sigmoid(logits))                                              # main.py:58
            labels.append(y)
            sizes.append(s)
        exhausted = self.check_status()                  # the epoch's one synchronisation: ids and chromosomes are checked once behind the loop
        if exhausted:
            print(f"warning: {exhausted} negatives could not be redrawn within 65536 trials and were returned equal to their positive")
        if n_batch == 0:
            return 0.0, 0.0, "", 0.0, 0.0
        auc, aupr, acc = _metrics(self, torch.cat(preds), torch.cat(labels), torch.cat(sizes))
        return float(bce_sum) / n_batch, float(rec_sum) / n_batch, acc, auc, aupr

    def train_epoch(self, edges, weights, batch_size: int = BATCH_SIZE, alpha: float = 1.0, beta: float = 0.001):
        """main.py:119-197: shuffle, floor(len / batch) steps; returns (bce mean, recon mean, acc, auc, aupr) as train.train_epoch does."""
        return self._epoch(edges, weights, batch_size, alpha, beta, True, None)

    @torch.no_grad()
    def eval_epoch(self, edges, weights, batch_size: int = BATCH_SIZE, alpha: float = 1.0, beta: float = 0.001, max_rows: int = 10000):
        """main.py:200-258: <= 10000 shuffled validation positives, fresh negatives, forward + loss only, in eval mode."""
        was = self.model.training
        self.model.eval()
        try:
            return self._epoch(edges, weights, batch_size, alpha, beta, False, max_rows)
        finally:
            self.model.train(was)


def run(config: dict, model_path: str, sizes, epochs: int, out: str, batch_size: int = BATCH_SIZE, lr: float = 1e-3, device: str = "cuda",
        log=print):
    from .train import MODEL_NAME, load_kmers
    sizes = sorted(int(k) for k in sizes)
    if sizes[0] < 2 or sizes[-1] > _lib.MAX_LONG_L:
        raise ValueError(f"--sizes must lie in 2 .. {_lib.MAX_LONG_L}")
    temp_dir = config["temp_dir"]
    chrom_range = np.load(os.path.join(temp_dir, "chrom_range.npy")).astype(np.int64)
    n2c_dict = np.load(os.path.join(temp_dir, "node2chrom.npy"), allow_pickle=True).item()
    N = int(sum(int(v[1] - v[0]) for v in chrom_range))
    node2chrom = np.full(N + 1, -1, dtype=np.int32)
    for k, v in n2c_dict.items():
        if 0 < int(k) <= N:
            node2chrom[int(k)] = int(v)
    model = torch.load(model_path, map_location=device, weights_only=False)                  # main.py:322, :685
    data, weight = load_kmers(temp_dir, sizes, float(config["quantile_cutoff_for_positive"]))
    weight = weight / np.mean(weight) * NEG_NUM                                              # main.py:594-595
    idx = np.arange(len(data))
    np.random.shuffle(idx)                                                                   # main.py:598
    split = int(0.8 * len(idx))
    known, _ = load_kmers(temp_dir, sizes, float(config["quantile_cutoff_for_unlabel"]))     # main.py:649-664
    sess = LongRowSession(model, known, node2chrom, chrom_range.astype(np.int32), neg_num=NEG_NUM, min_dis=int(config["min_distance"]), lr=lr)
    os.makedirs(out, exist_ok=True)
    for epoch in range(epochs):
        t0 = time.time()
        bce, rec, acc, auc, aupr = sess.train_epoch(data[idx[:split]], weight[idx[:split]], batch_size)
        log(f"[ Epoch {epoch} of {epochs} ]  - (Training)   bce: {bce:7.4f}, recon: {rec:7.4f} acc: {acc}, auc: {auc}, aupr: {aupr}, "
            f"elapse: {time.time() - t0:3.3f} s")
        t0 = time.time()
        vb, vr, vacc, vauc, vaupr = sess.eval_epoch(data[idx[split:]], weight[idx[split:]], batch_size)
        log(f"  - (Validation-hyper) bce: {vb:7.4f}, recon: {vr:7.4f},  acc: {vacc}, auc: {vauc}, aupr: {vaupr}, elapse: {time.time() - t0:3.3f} s")
        torch.save({"model_link": model.state_dict(), "epoch": epoch}, os.path.join(out, MODEL_NAME))      # main.py:316-321
        torch.save(model, os.path.join(out, "model2load"))                                                  # main.py:322
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="./config.JSON")
    ap.add_argument("--model", default=None, help="a pickled model (default: temp_dir/model2load)")
    ap.add_argument("--sizes", type=int, nargs="+", required=True, help="hyperedge sizes to train on, 2 .. 32 (all_<k>_counter.npy of temp_dir)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=BATCH_SIZE)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("-o", "--output", default=None, help="directory for the checkpoint and model2load (default: temp_dir)")
    a = ap.parse_args(argv)
    config = U.get_config(a.config)
    model_path = a.model or "model2load"
    if not os.path.exists(model_path):
        model_path = os.path.join(config["temp_dir"], model_path)
    run(config, model_path, a.sizes, a.epochs, a.output or config["temp_dir"], a.batch_size, a.lr)


if __name__ == "__main__":
    main()
