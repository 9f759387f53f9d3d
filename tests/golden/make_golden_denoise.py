#!/usr/bin/env python3
"""Generate the gd_* fixtures of the denoised contact maps by running the REAL reference script (Code/denoise_contact.py).

Runs only in the build container (needs the reference; see make_golden.py, whose helpers it imports and which it does not change).
The script has no functions to call: its top-level statements are exec'd from its AST, in order, in a scratch directory that holds
config.JSON and Temp/{model2load, chrom_range.npy, node2bin.npy, intra_adj.npy}, with these stand-ins:

  * h5py records every create_dataset (path -> array); seaborn / matplotlib do nothing (the plots are out of scope);
  * the CPU-only ``torch.cuda.set_device`` statement (:104) is skipped; ``task_mode`` (:106) is set per case;
  * ``torch.load`` (:99) unpickles whole models, the default of the torch releases the reference was written for
    (TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD);
  * ``transformer`` (:105) wraps scikit-learn's QuantileTransformer(n_quantiles=1000, 'uniform') and records each input and output.
    It passes subsample=None only when the column has more than 10 000 values -- where scikit-learn's default would fit on a random
    sample -- so every chromosome of at most 100 bins is the reference exactly;
  * the chromosome loop (:147-208) ends with a hook that records the chromosome's probabilities, gaps and pixels.

Inputs are regenerated from seeds (tests/denoise_ref.py: fixture_intra, fixture_node2bin); the models are the reference-pickled tiny
models (ref_model2load_tiny_{adj,table}) and, for the mid layout, a reference-initialised table model.

Usage:  python tests/golden/make_golden_denoise.py
"""
import ast
import io
import os
import shutil
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import REF, build_ref, import_reference, redirect_stderr_null, synth  # noqa: E402

sys.path.insert(0, ROOT)
from tests.denoise_ref import FIXTURE_LAYOUTS, FIXTURE_RES, fixture_intra, fixture_node2bin  # noqa: E402

# name -> (layout, model, min_distance, task_mode, intra seed)
CASES = {
    "tiny_table_md2": ("tiny", "table", 2, "class", 81),
    "tiny_adj_md0": ("tiny", "adj", 0, "class", 82),
    "tiny_table_regress": ("tiny", "table", 2, "regress", 83),
    "mid_table_md2": ("mid", "refinit", 2, "class", 84),
}
MID_MODEL = (16, 85)           # embed_dim, weight seed of the mid layout's reference-initialised table model


class _Nothing:
    """Accepts any attribute access and call (the plotting calls)."""

    def __getattr__(self, name):
        return _Nothing()

    def __call__(self, *a, **k):
        return _Nothing()


def _stub_plotting():
    mpl = types.ModuleType("matplotlib")
    mpl.use = lambda *a, **k: None
    plt = types.ModuleType("matplotlib.pyplot")
    plt.__getattr__ = lambda name: _Nothing()
    mpl.pyplot = plt
    sns = types.ModuleType("seaborn")
    sns.__getattr__ = lambda name: _Nothing()
    sys.modules.update({"matplotlib": mpl, "matplotlib.pyplot": plt, "seaborn": sns})


class _H5Group:
    def __init__(self, rec, path):
        self.rec, self.path = rec, path

    def create_group(self, name):
        return _H5Group(self.rec, self.path + name + "/")

    def create_dataset(self, name, data=None, dtype=None):
        self.rec[self.path + name] = np.asarray(data)


def _stub_h5py(rec):
    h5 = types.ModuleType("h5py")
    h5.File = lambda path, mode="r": _H5Group(rec, "")
    h5.special_dtype = lambda **k: None
    sys.modules["h5py"] = h5


class RecordingTransformer:
    """QuantileTransformer(n_quantiles=1000, output_distribution='uniform') as :105 builds it; subsample=None above 10 000 values."""

    def __init__(self):
        self.calls = []

    def fit_transform(self, X):
        from sklearn.preprocessing import QuantileTransformer
        kw = {"subsample": None} if X.shape[0] > 10000 else {}
        out = QuantileTransformer(n_quantiles=1000, output_distribution="uniform", **kw).fit_transform(X)
        self.calls.append((np.array(X, copy=True), np.array(out, copy=True)))
        return out


def run_reference(case):
    layout, model, min_dis, task_mode, seed = CASES[case]
    num = FIXTURE_LAYOUTS[layout]
    M, U = import_reference()
    work = tempfile.mkdtemp(prefix="matcha_gd_")
    temp, run = os.path.join(work, "Temp"), os.path.join(work, "run")
    os.makedirs(temp)
    os.makedirs(run)
    node2bin, names = fixture_node2bin(num)
    np.save(os.path.join(temp, "node2bin.npy"), node2bin, allow_pickle=True)
    np.save(os.path.join(temp, "chrom_range.npy"), np.asarray(synth.chrom_range(num)))
    np.save(os.path.join(temp, "intra_adj.npy"), fixture_intra(num, seed))
    if model == "refinit":
        clf, *_ = build_ref(M, num, MID_MODEL[0], "table", MID_MODEL[1])
        torch.save(clf, os.path.join(temp, "model2load"))
    else:
        shutil.copy(os.path.join(HERE, f"ref_model2load_tiny_{model}"), os.path.join(temp, "model2load"))
    import json
    with open(os.path.join(run, "config.JSON"), "w") as f:
        json.dump({"temp_dir": temp, "resolution": FIXTURE_RES, "chrom_list": names, "min_distance": min_dis}, f)

    datasets, per_chrom, transformer = {}, [], RecordingTransformer()
    _stub_plotting()
    _stub_h5py(datasets)
    tree = ast.parse(open(os.path.join(REF, "denoise_contact.py")).read())
    hook = ast.parse("_record(i)").body[0]
    glb = {"__name__": "denoise_contact"}

    def record(i):
        per_chrom.append({"proba": np.array(glb["proba"], copy=True), "gap1": np.array(glb["gap1"]), "gap2": np.array(glb["gap2"]),
                          "balanced": np.array(glb["value"], copy=True), "pairs": np.array(glb["pair_wise"], copy=True)})

    glb["_record"] = record
    cwd = os.getcwd()
    os.environ["TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD"] = "1"
    os.chdir(run)
    try:
        with redirect_stdout(io.StringIO()), redirect_stderr_null():
            for node in tree.body:
                src = ast.unparse(node)
                if src.startswith("torch.cuda.set_device("):
                    continue                                         # :104 (CPU-only run)
                if isinstance(node, ast.For) and ast.unparse(node.iter) == "range(len(chrom_name))":
                    node.body.append(hook)                           # the chromosome loop (:147), not the bins loop (:125)
                exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), os.path.join(REF, "denoise_contact.py"),
                             "exec"), glb)
                if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "transformer" for t in node.targets):
                    glb["transformer"] = transformer
                if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "task_mode" for t in node.targets):
                    glb["task_mode"] = task_mode
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    assert len(transformer.calls) == 3 * len(num) and len(per_chrom) == len(num)
    for c, rec in enumerate(per_chrom):
        n = num[c]
        for k, name in enumerate(("my", "origin_part", "my_proba")):
            x, y = transformer.calls[3 * c + k]
            rec[name], rec[name + "_q"] = x.reshape(n, n), y.reshape(n, n)
    return num, min_dis, task_mode, per_chrom, datasets


def main():
    torch.set_num_threads(4)
    for case in CASES:
        num, min_dis, task_mode, per_chrom, datasets = run_reference(case)
        head = {"num": np.asarray(num, dtype=np.int64), "min_dis": np.int64(min_dis), "task_mode": np.array(task_mode),
                "res": np.int64(FIXTURE_RES), "seed": np.int64(CASES[case][4])}
        head.update({"ds/" + k: v for k, v in datasets.items()})
        files = {f"gd_{case}.npz": dict(head)}
        for c, rec in enumerate(per_chrom):
            # the mid layout: one file per chromosome (every committed file stays under 1 MiB); my_proba_q only up to 100 bins
            out = files[f"gd_{case}.npz"] if num[c] <= 64 else files.setdefault(f"gd_{case}_c{c}.npz", {})
            for k, v in rec.items():
                if k == "pairs" or (k == "my_proba_q" and num[c] > 100):
                    continue
                out[f"{k}_c{c}"] = v
        for name, out in files.items():
            path = os.path.join(HERE, name)
            np.savez_compressed(path, **out)
            print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
