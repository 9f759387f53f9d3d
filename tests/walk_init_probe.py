"""What a short matcha_amd.train.run of the table front end computes from fixed seeds, as arrays that can be compared bit for bit: the
recorded answer of the commit BEFORE the walk initialisation (tests/golden/walk_parent_random_init.npz) pins ``table_init="random"`` to it.

    python -m tests.walk_init_probe out.npz        # on a GPU; run on the parent commit to write the golden (it passes no table_init)

``probe`` runs train.run (d = 64, layout tiny, 1 + 1 epochs of 2 batches, deterministic table gradient) and records
  * at the first training epoch, before any step: the table, the eval-mode logits of the freshly initialised model on fixed rows (they
    depend on every parameter), and the states of torch's CPU generator, torch's device generator and numpy's global generator -- what
    building the model consumed from each;
  * after the run: the logits on the same rows (every training step's logits went into them).
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROWS = [[1, 5, 9], [2, 20, 0], [3, 4, 33], [7, 50, 51], [10, 11, 0], [6, 30, 45]]


def _numpy_state():
    s = np.random.get_state()
    return np.concatenate([np.asarray(s[1], dtype=np.uint32), np.asarray([s[2]], dtype=np.uint32)])


def probe(tmp, **run_kw):
    from matcha_amd import train as T
    import Modules  # noqa: F401
    from tests.test_train_driver import _write_temp_dir
    cfg, num = _write_temp_dir(str(tmp), m=600, d=64)
    x = torch.tensor(ROWS)
    out = {}
    real_train = T.train

    def logits(model):
        was = model.training
        model.eval()
        with torch.no_grad():
            lg = model(x).detach().float().cpu().numpy().copy()
        model.train(was)
        return lg

    def spy(sess, *a, **k):
        if "table" not in out:
            states = (torch.get_rng_state().numpy().copy(), torch.cuda.get_rng_state().cpu().numpy().copy(), _numpy_state())
            out["table"] = sess.model.node_embedding.weight.detach().cpu().numpy().copy()
            out["logits_init"] = logits(sess.model)
            torch.set_rng_state(torch.from_numpy(states[0]))           # (the forward above is eval-mode; put back what it may have drawn)
            torch.cuda.set_rng_state(torch.from_numpy(states[1]))
            out["torch_cpu_state"], out["torch_dev_state"], out["numpy_state"] = states
        return real_train(sess, *a, **k)
    T.train = spy
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        model = T.run(cfg, front_end="table", epochs1=1, epochs2=1, batches_per_epoch=2, emb_path=os.path.join(str(tmp), "emb.npy"),
                      log=lambda *_: None, deterministic=True, **run_kw)
    finally:
        T.train = real_train
    out["logits_trained"] = logits(model)
    return out


def main(path):
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        first, second = probe(a), probe(b)
    same = {k: bool(np.array_equal(first[k], second[k])) for k in first}
    print("two runs agree:", same)
    np.savez(path, repeatable=np.asarray([same[k] for k in sorted(same)]), keys=np.asarray(sorted(same)), **first)


if __name__ == "__main__":
    main(sys.argv[1])
