"""The inference forward for rows of 9 to 32 nodes (matcha_forward_long; Classifier.forward at 9 <= L <= 32) on the device: parity with the
real reference (tests/golden/g12_long_rows.npz), fp32 grade against the fp64 oracle (tests/fp64_grade.py as it is, K = 8) with the
three-product witness rejected by the same bound, the long kernels against the L <= 8 kernels on identical input, shape edges, the
row's width, status and refusals, the untouched L <= 8 path, and the `predict multiway` consumer.  GPU only (-m gpu)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR, synth
from oracle import hypersagnn as O
from tests import fp64_grade as G
from tests.helpers import GOLD, gold, logit_err, oracle_state
from tests.test_cpu_long_rows import WIDTHS, golden_oracle
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
LONG_PLAN = {"long_plan_count_kernel", "long_plan_scan_kernel", "long_plan_fill_kernel"}
LONG = LONG_PLAN | {"attn_long_kernel"}
SHORT_ONLY = {"fused_fwd32_kernel", "fused_fwd32h_kernel", "attn_fwd_kernel", "attn_fwd_wide_kernel", "enc128_fwd_kernel", "plan_small_kernel",
              "row_fill_kernel"}

_MODELS = {}


def model(layout, d, mode, seed):
    """(clf in eval mode on the device, sd, fe): one model per configuration for the whole module."""
    key = (layout, d, mode, seed)
    if key not in _MODELS:
        num = synth.LAYOUTS[layout]
        _, fe, sd = oracle_state(num, d, mode, seed)
        clf, _ = hip_model(num, d, mode, seed, sd=sd)
        _MODELS[key] = (clf.eval(), sd, fe)
    return _MODELS[key]


def rows_of(rng, N, ks, L):
    """int64 [len(ks), L]: row b holds ks[b] distinct sorted ids of 1..N, then zeros."""
    x = np.zeros((len(ks), L), dtype=np.int64)
    for b, k in enumerate(ks):
        x[b, :k] = np.sort(rng.choice(N, size=k, replace=False) + 1)
    return x


def grade_batch(rng, N, L, B=65):
    """k = L, 2, 1, 0, 9, then k uniform in [2, L]."""
    ks = [L, 2, 1, 0, 9] + [int(k) for k in rng.integers(2, L + 1, size=B - 5)]
    return rows_of(rng, N, ks[:B], L)


def refs(sd, fe, x):
    y, w = np.zeros(len(x), dtype=np.float32), np.ones(len(x), dtype=np.float32)
    return G.references(sd, fe, x, y, w, backward=False)


def run(clf, x):
    """(logits float64 [B], {kernel: launches}) of model(x) under no_grad."""
    with torch.no_grad(), _lib.launch_log() as log:
        lg = clf(torch.from_numpy(x))
        torch.cuda.synchronize()
    assert lg.shape == (len(x), 1)
    return lg.cpu().numpy().reshape(-1).astype(np.float64), {k for k, n in log.counts.items() if n > 0}


def c_forward(clf, x, long_rows, training=0, forward_only=1):
    """matcha_forward_long / matcha_forward called directly (forward-only workspace): (rc, logits, kernels)."""
    rt = clf._runtime()
    lib = rt.lib
    with torch.no_grad():
        opts, _ = clf._opts(rt, False)
    opts.training, opts.forward_only = training, forward_only
    opts.status = rt.status.data_ptr()
    xt = torch.from_numpy(x).cuda().contiguous()
    B, L = xt.shape
    ws = rt.workspace(B, L, forward_only=True, long_rows=long_rows)
    logits = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    losses = torch.zeros(3, dtype=torch.float32, device="cuda")
    with _lib.launch_log() as log:
        if long_rows:
            rc = lib.matcha_forward_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), B, L, _lib.ptr(logits),
                                         _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream())
        else:
            rc = lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), B, L, None, None,
                                    _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream())
        torch.cuda.synchronize()
    return rc, logits.cpu().numpy().astype(np.float64), {k for k, n in log.counts.items() if n > 0}


# ---- 1. reference parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_reference_parity_on_long_rows(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    g = gold("g12_long_rows.npz")
    clf = torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False).eval()
    for L in WIDTHS:
        lg, ran = run(clf, g[f"rows_L{L}"].astype(np.int64))
        e = logit_err(lg, g[f"logit_{mode}_L{L}"])
        print(f"{mode} L {L}: logit_err {e:.2e}")
        assert e <= TOL, (mode, L, e)
        assert LONG <= ran and not (ran & {"fused_fwd32_kernel", "fused_fwd32h_kernel", "attn_fwd_kernel"}), sorted(ran)


# ---- 2. fp32 grade ----------------------------------------------------------------------------------------------------------------------------
GRADE_CASES = [("hg38_1mb", 64, "table", 181), ("c1", 128, "adj", 182), ("c1", 256, "table", 183), ("tiny", 16, "adj", 184)]


@pytest.mark.parametrize("L", [9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_long_rows_at_fp32_grade(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    x = grade_batch(np.random.default_rng(seed + L), N, L)
    assert x.shape == (65, L) and [int(k) for k in (x[:5] != 0).sum(1)] == [L, 2, 1, 0, 9]
    ref = refs(sd, fe, x)
    lg, ran = run(clf, x)
    assert LONG <= ran and not (ran & SHORT_ONLY), sorted(ran)
    assert lg[3] == 0.0                                                       # the all-padding row: logit 0, like the reference
    G.assert_grade(f"long {layout} d{d} {mode} L{L}", G.logit_rows(lg, ref, G.K))
    # the same bound rejects the three-product witness
    y, w = np.zeros(len(x), dtype=np.float32), np.ones(len(x), dtype=np.float32)
    wit = G.oracle_step(sd, fe, x, y, w, ops=O.Ops(mm=G.three_product_mm, bmm=G.three_product_mm), backward=False)
    rows = G.logit_rows(wit.logits, ref, G.K)
    print("witness e/noise", [round(r.ratio, 1) for r in rows])
    assert not all(r.ok for r in rows), [(r.what, r.ratio) for r in rows]


# ---- 3. the long kernels against the existing ones ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,mode,seed", [("hg38_1mb", 64, "table", 181), ("c1", 128, "adj", 182)])
@pytest.mark.parametrize("L", [8, 5])
def test_long_kernels_against_the_short_path(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    rng = np.random.default_rng(seed + 40 + L)
    ks = [L, 2, 1, 0] + [int(k) for k in rng.integers(1, L + 1, size=253)]
    x = rows_of(rng, N, ks, L)
    ref = refs(sd, fe, x)
    rc_l, lg_l, ran_l = c_forward(clf, x, True)
    rc_s, lg_s, ran_s = c_forward(clf, x, False)
    assert rc_l == 0 and rc_s == 0
    assert LONG <= ran_l and not (ran_l & SHORT_ONLY) and not (ran_s & LONG), (sorted(ran_l), sorted(ran_s))
    G.assert_grade(f"long kernels {layout} d{d} L{L}", G.logit_rows(lg_l, ref, G.K))
    G.assert_grade(f"short kernels {layout} d{d} L{L}", G.logit_rows(lg_s, ref, G.K))


# ---- 4. shape edges ---------------------------------------------------------------------------------------------------------------------------
EDGE = ("hg38_1mb", 64, "table", 181)


def _graded(label, x):
    clf, sd, fe = model(*EDGE)
    lg, ran = run(clf, x)
    assert LONG <= ran and not (ran & SHORT_ONLY), sorted(ran)
    G.assert_grade(label, G.logit_rows(lg, refs(sd, fe, x), G.K))
    return lg


@pytest.mark.parametrize("B", [1, 3, 64, 65, 257])
def test_batch_sizes_at_width_17(B):
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(400 + B)
    ks = ([17] + [int(k) for k in rng.integers(1, 18, size=B - 1)])[:B]
    _graded(f"B {B} L 17", rows_of(rng, N, ks, 17))


def test_full_rows_4099_by_32():
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(432)
    x = np.sort(np.argsort(rng.random((4099, N)), axis=1)[:, :32] + 1, axis=1).astype(np.int64)
    _graded("B 4099 L 32 k 32", x)


def test_predict_chunk_shape_one_long_row():
    """4 098 rows of k = 3 and one of k = 25 at width 25: what a `predict multiway` chunk with one long line looks like."""
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(425)
    ks = [3] * 4099
    ks[2500] = 25
    _graded("B 4099 L 25, one long row", rows_of(rng, N, ks, 25))


def test_pads_inside_rows_repeated_ids_and_empty_runs():
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(417)
    L, B = 17, 300
    ks = [int(k) for k in rng.integers(1, L + 1, size=B)]
    x = rows_of(rng, N, ks, L)
    for b in range(0, B, 3):                                  # pads anywhere in the row: the real ids keep their order, the slots move
        slots = np.sort(rng.choice(L, size=ks[b], replace=False))
        row = np.zeros(L, dtype=np.int64)
        row[slots] = x[b, :ks[b]]
        x[b] = row
    x[1, :4] = [7, 9, 9, 30]                                  # a repeated id in a row
    x[4, :L] = np.sort(rng.choice(N, size=L, replace=False) + 1)
    x[4, 5] = x[4, 11]                                        # ... and in a full row, out of order
    x[100:170] = 0                                            # a run of 70 all-padding rows in the middle of the batch
    lg = _graded("pads inside rows, repeated ids, empty run", x)
    assert (lg[100:170] == 0.0).all()


# ---- 5. the width is honoured -----------------------------------------------------------------------------------------------------------------
def test_width_is_honoured():
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(505)
    base = rows_of(rng, N, [9] + [int(k) for k in rng.integers(2, 10, size=63)], 9)
    oracle = {}
    for L in (9, 16, 32):
        x = np.pad(base, ((0, 0), (0, L - 9)))
        ref = refs(sd, fe, x)
        lg, ran = run(clf, x)
        assert LONG <= ran
        G.assert_grade(f"width {L}", G.logit_rows(lg, ref, G.K))
        oracle[L] = ref.r32a.logits
    for a, b in ((9, 16), (16, 32), (9, 32)):                 # asserted on the oracle's numbers: a test that pads to the wrong width fails visibly
        gap = logit_err(oracle[a], oracle[b])
        print(f"width {a} vs {b}: logit_err {gap:.3f}")
        assert gap > 100 * TOL, (a, b, gap)


# ---- 6. status and refusals -------------------------------------------------------------------------------------------------------------------
def test_status_and_refusals():
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(606)
    x = rows_of(rng, N, [9, 4, 12, 2], 12)
    bad = x.copy()
    bad[2, 7] = N + 1
    with torch.no_grad():
        with pytest.raises(IndexError):
            clf(torch.from_numpy(bad))
        clf(torch.from_numpy(x))                              # the status word was cleared
        with pytest.raises(IndexError):
            with clf.deferred_id_check():
                clf(torch.from_numpy(bad))                    # no read-back here ...
                lg = clf(torch.from_numpy(x))                 # ... nor here: raised at the end of the block
        assert lg.shape == (4, 1)
        with pytest.raises(ValueError, match="32"):
            clf(torch.zeros(2, 33, dtype=torch.long))
    x9 = torch.from_numpy(rows_of(rng, N, [9, 3], 9))
    with _lib.launch_log() as log:
        with pytest.raises(NotImplementedError, match="inference-only"):
            clf(x9)                                           # grad enabled, trainable parameters
        clf.train()
        try:
            with torch.no_grad(), pytest.raises(NotImplementedError, match="inference-only"):
                clf(x9)
        finally:
            clf.eval()
    assert not log.counts, log.counts
    for training, forward_only in ((1, 1), (0, 0)):
        rc, lg, ran = c_forward(clf, x, True, training=training, forward_only=forward_only)
        assert rc == -22 and not ran and np.isnan(lg).all()
        assert "inference-only" in _lib.load().matcha_last_error().decode()


# ---- 7. the existing path is untouched ----------------------------------------------------------------------------------------------------------
def test_short_rows_run_no_long_kernel():
    from matcha_amd.engine import Trainer
    clf, sd, fe = model(*EDGE)
    x, y, w = G.make_case_batch(EDGE[0], [2, 5, 8], 64, 707, 8)
    assert x.shape[1] == 8
    lg, ran = run(clf, x)
    assert not (ran & LONG) and ran & {"fused_fwd32_kernel", "fused_fwd32h_kernel"}, sorted(ran)
    clf2, _ = hip_model(synth.LAYOUTS[EDGE[0]], 64, "table", EDGE[3], sd=sd)
    tr = Trainer(clf2, lr=1e-3)
    with _lib.launch_log() as log:
        tr.step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda())
        torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    assert ran and not (ran & LONG), sorted(ran)


# ---- 8. the consumer --------------------------------------------------------------------------------------------------------------------------
def test_predict_multiway_cli_on_long_lines(tmp_path):
    import Modules  # noqa: F401
    g = gold("g6_inference_tiny.npz")
    bin2node = {str(k): int(v) for k, v in zip(g["bin_keys"], g["bin_vals"])}
    node2bin = {v: k for k, v in bin2node.items()}
    names, res = [str(n) for n in g["names"]], int(g["res"])
    N = int(np.sum(synth.LAYOUTS["tiny"]))
    rng = np.random.default_rng(808)
    sizes = [25, 2, 1, 9] + [int(k) for k in rng.integers(2, 26, size=26)]
    lines = [np.sort(rng.choice(N, size=k, replace=False) + 1) for k in sizes]
    kept = [[int(v) for v in r] for r in lines if len(r) > 1]

    def write(path, rows):
        with open(path, "w") as f:
            for r in rows:
                f.write("\t".join(node2bin[int(v)] for v in rng.permutation(r)) + "\n")

    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    np.save(os.path.join(temp, "bin2node.npy"), bin2node, allow_pickle=True)
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": res, "chrom_list": names, "min_distance": 2}, f)
    inp, out = os.path.join(tmp_path, "in.txt"), os.path.join(tmp_path, "out.txt")
    write(inp, lines)
    PR.main(["multiway", "-i", inp, "-o", out, "--config", cpath])
    proba = np.loadtxt(out).reshape(-1)
    assert proba.shape == (len(kept),) == (29,)

    P, fe = golden_oracle("table")

    def oracle_proba(rows):
        x = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int64)
        for i, r in enumerate(rows):
            x[i, :len(r)] = r
        with torch.no_grad():
            lg, _ = O.classifier_forward(P, fe, torch.from_numpy(x), random_chrom=0)
        return torch.sigmoid(lg.reshape(-1)).numpy()

    assert np.abs(proba - oracle_proba(kept)).max() <= TOL            # one chunk: every row at width 25
    # per chunk width: chunks of 7 rows are padded to their own longest row
    clf = torch.load(os.path.join(temp, "model2load"), map_location="cuda", weights_only=False)
    got = torch.sigmoid(torch.from_numpy(PR.predict(clf, kept, batch_size=7))).numpy().reshape(-1)
    want = np.concatenate([oracle_proba(kept[j:j + 7]) for j in range(0, len(kept), 7)])
    assert np.abs(got - want).max() <= TOL
    assert np.abs(got - proba).max() > 100 * TOL                       # (and that is another result than the single chunk's)
    # a 33-locus line fails with its line number, before anything is scored
    write(inp, lines[:10] + [np.arange(1, 34)] + lines[10:])
    os.remove(out)
    with pytest.raises(ValueError, match=r"line 11 has 33 distinct bins"):
        PR.main(["multiway", "-i", inp, "-o", out, "--config", cpath])
    assert not os.path.exists(out)
