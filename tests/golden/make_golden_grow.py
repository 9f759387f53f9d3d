#!/usr/bin/env python3
"""Generate g17_grow_tiny.npz: cluster growth driven by the REAL reference.

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
For the two reference-pickled tiny models (ref_model2load_tiny_{table,adj}) and the four cases of tests/grow_ref.py::G17_CASES (region,
beam, min_gap, seed sizes, max_size, width W) it runs the reference's own beam search: tests/grow_ref.py's rule with
predict_multiway.py's ``predict`` (:74-87) as the score, one chunk of at most 1 536 rows per call whose width is pinned to W by one
filler row of W nodes (its logit is dropped): a logit depends on its chunk's width (SURVEY.md headline fact 7).  A chunk whose rows all
have W ids is handed over as an integer array (an object array of equal-length lists breaks the reference's np2tensor_hyper).  It stores

  seeds_c<i>                 the seeds, zero-padded (int16 [A, S]),
  beam_<mode>_c<i>_t<t>      the beam that enters step t, for the seeds that step runs on (int16 [A_t, B_t, S_t]),
  logit_<mode>_c<i>_t<t>     the reference's logit of every candidate of that beam in global-rank order (float32 [A_t B_t n]); NaN for the
                             candidates of an empty slot, which are not scored.

Asserted here: over all steps of a (case, mode) at most G17_NEAR valid non-twin candidates lie within the project's tolerance (1e-4 of
the seed's max |logit|) of the seed's B-th best logit, so the teacher-forced comparison of tests/test_hip_grow.py is an exact set
comparison almost everywhere.  If another seed base is ever needed, choose one for which the reference alone meets that condition.

Usage:  python tests/golden/make_golden_grow.py
"""
import io
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import import_reference, redirect_stderr_null, ref_functions, synth  # noqa: E402
from tests import complete_ref as CR  # noqa: E402
from tests import grow_ref as GR  # noqa: E402

CHUNK = 1536


def main():
    torch.set_num_threads(4)
    M, U = import_reference()
    from torch.nn.utils.rnn import pad_sequence
    num = synth.LAYOUTS["tiny"]
    n_nodes = int(np.sum(num))
    common = dict(np=np, os=os, sys=sys, math=math, torch=torch, print=lambda *a, **k: None, trange=range,
                  np2tensor_hyper=U.np2tensor_hyper, pad_sequence=pad_sequence, device=torch.device("cpu"))
    pm = ref_functions("predict_multiway.py", {"predict"}, dict(common))
    out = {"num": np.asarray(num, dtype=np.int64), "seed_base": np.int64(GR.G17_SEED)}
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    for i, ((lo, hi), B, gap, sizes, max_size, W) in enumerate(GR.G17_CASES):
        n = hi - lo
        seeds = GR.g17_seeds(i, n_nodes)
        assert [len(s) for s in seeds] == list(sizes) and max_size <= W and 1 <= lo and hi <= n_nodes + 1
        out[f"seeds_c{i}"] = CR.padded(seeds).astype(np.int16)
        filler = list(range(1, W + 1))                                 # W nodes: pins the chunk's width
        for mode in ("table", "adj"):
            with redirect_stdout(io.StringIO()), redirect_stderr_null():
                clf = torch.load(os.path.join(HERE, f"ref_model2load_tiny_{mode}"), map_location="cpu", weights_only=False)

            def score(rows):
                lists = [[int(v) for v in r if v != 0] for r in rows]
                todo = [k for k, ids in enumerate(lists) if len(ids) >= 2]           # an empty slot's candidate is its free id alone
                logits = np.full(len(lists), np.nan, dtype=np.float32)
                for c0 in range(0, len(todo), CHUNK - 1):
                    part = todo[c0:c0 + CHUNK - 1]
                    chunk = [lists[k] for k in part] + [filler]
                    if all(len(ids) == W for ids in chunk):
                        samples = np.asarray(chunk, dtype=np.int64)
                    else:
                        samples = np.asarray(chunk, dtype=object)
                    assert len(samples) <= CHUNK
                    with redirect_stdout(io.StringIO()), redirect_stderr_null():
                        got = np.asarray(pm["predict"](clf, samples)).reshape(-1).astype(np.float32)
                    assert got.shape == (len(part) + 1,) and np.isfinite(got).all()
                    logits[part] = got[:-1]
                return logits

            cur = {a: [seeds[a]] for a in range(len(seeds))}
            near, gaps = 0, []
            for t, active, B_t, S_t in GR.g17_steps(i):
                beam = np.stack([CR.padded(cur[a], S_t) for a in active])
                assert beam.shape == (len(active), B_t, S_t)
                rows, bad, tw = GR.candidates(beam, lo, n, gap, W)
                logits = score(rows)
                res = GR.step(beam, lo, n, gap, W, B, lambda r: logits)
                out[f"beam_{mode}_c{i}_t{t}"] = beam.astype(np.int16)
                out[f"logit_{mode}_c{i}_t{t}"] = logits
                seg = B_t * n
                for k, a in enumerate(active):
                    ok = ~(bad | tw)[k * seg:(k + 1) * seg]
                    lg = np.sort(logits[k * seg:(k + 1) * seg][ok].astype(np.float64))[::-1]
                    assert not np.isnan(lg).any() and res["count"][k] == min(B, len(lg))
                    if len(lg) > B:
                        m = GR.G17_TOL * np.abs(lg).max()
                        near += int((np.abs(lg - lg[B - 1]) <= m).sum()) - 1
                        gaps.append((lg[B - 1] - lg[B]) / np.abs(lg).max())
                    cur[a] = [CR.leading_ids(r) for r in res["beam"][k]]
            assert near <= GR.G17_NEAR, (i, mode, near)
            print(f"case {i} (region [{lo}, {hi}), beam {B}, min_gap {gap}, seeds {sizes}, max_size {max_size}, W {W}) {mode}: "
                  f"{len(GR.g17_steps(i))} steps, {near} candidates within tolerance of a B-th logit, gap behind the B-th: "
                  f"min {min(gaps):.1e} median {np.median(gaps):.1e}")
    path = os.path.join(HERE, "g17_grow_tiny.npz")
    np.savez_compressed(path, **out)
    print("g17_grow_tiny.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
