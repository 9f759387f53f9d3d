"""Outlier identification on the device: Classifier.locus_scores / matcha_locus_scores (head_scores_kernel) against the real
reference's per-position scores (tests/golden/g19_locus_scores.npz), at fp32 grade against the fp64 oracle (tests/fp64_grade.py::row as it
is, K = 8), its exact structure, its order against the twin's rule, the kernels it runs and what it leaves untouched; matcha_outlier_plant
(outlier_plant_kernel) bit for bit against the plain-Python twin (tests/outlier_ref.py); the benchmark's counts against a numpy recount; the
`predict outliers` consumer.  GPU only (-m gpu)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR, synth
from matcha_amd.outlier import OutlierPlanter, outlier_benchmark
from matcha_amd.sampler import HyperedgeSet
from tests import fp64_grade as G
from tests import outlier_ref as OR
from tests.helpers import GOLD, gold
from tests.test_cpu_outlier import GRADE_CASES, WIDTHS, WITNESS_CASES, grade_rows, score_refs, scores_batch, witness_scores
from tests.test_hip_long_rows import LONG_PLAN, SHORT_ONLY, c_forward, model, rows_of
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

HEAD = "head_scores_kernel"
NOT_HERE = SHORT_ONLY | {"head_fwd_kernel", "attn_long_prob_kernel", "expand_embedding_kernel"}
EDGE = ("hg38_1mb", 64, "table", 181)


def scores_of(clf, x, lowest=0):
    """(LocusScores, kernels) of clf.locus_scores(x, lowest) under no_grad."""
    with torch.no_grad(), _lib.launch_log() as log:
        res = clf.locus_scores(torch.from_numpy(x), lowest=lowest)
        torch.cuda.synchronize()
    assert res.logits.shape == (len(x), 1) and res.scores.shape == x.shape
    assert (res.order is None) if lowest == 0 else (res.order.shape == (len(x), lowest) and res.order.dtype == torch.int64)
    return res, {k for k, n in log.counts.items() if n > 0}


def c_scores(clf, x, lowest, ws=None, training=0):
    """matcha_locus_scores called directly on NaN- / garbage-filled outputs: (rc, scores, logits, order, kernels)."""
    rt = clf._runtime()
    with torch.no_grad():
        opts, _ = clf._opts(rt, False)
    opts.training, opts.forward_only = training, 1
    opts.status = rt.status.data_ptr()
    xt = torch.from_numpy(x).cuda().contiguous()
    B, L = xt.shape
    ws = rt.workspace(B, L, long_rows=True) if ws is None else ws
    scores = torch.full((B, L), float("nan"), dtype=torch.float32, device="cuda")
    logits = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    order = torch.full((B, lowest), -77, dtype=torch.long, device="cuda") if lowest else None
    losses = torch.zeros(3, dtype=torch.float32, device="cuda")
    with _lib.launch_log() as log:
        rc = rt.lib.matcha_locus_scores(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), B, L, _lib.ptr(scores),
                                        _lib.ptr(logits), lowest, _lib.ptr(order), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream())
        torch.cuda.synchronize()
    return rc, scores, logits, order, {k for k, n in log.counts.items() if n > 0}


# ---- 1. reference parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_reference_parity_of_the_scores(mode):
    """max|scores - ref * mask| <= 1e-4 max|ref|, the logits within the same bound of the fixture's."""
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    g = gold("g19_locus_scores.npz")
    clf = torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False).eval()
    for L in WIDTHS:
        x = g[f"rows_L{L}"].astype(np.int64)
        ref = g[f"scores_{mode}_L{L}"].astype(np.float64) * (x != 0)
        zref = g[f"logits_{mode}_L{L}"].astype(np.float64)
        res, ran = scores_of(clf, x, lowest=3)
        e_s = float(np.abs(res.scores.cpu().numpy() - ref).max() / np.abs(ref).max())
        e_z = float(np.abs(res.logits.cpu().numpy().reshape(-1) - zref).max() / np.abs(zref).max())
        print(f"{mode} L {L}: scores {e_s:.2e}, logits {e_z:.2e} of max|ref|")
        assert e_s <= 1e-4 and e_z <= 1e-4, (mode, L, e_s, e_z)
        assert LONG_PLAN | {HEAD, "attn_long_kernel"} <= ran and not (ran & NOT_HERE), sorted(ran)


# ---- 2. fp32 grade ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 8, 9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_scores_at_fp32_grade(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    for B in (17, 33):                                           # a full 16-hyperedge block and a partial one; two full ones and a partial one
        x = scores_batch(np.random.default_rng(seed + 100 * L + B), N, L, B)
        ks = (x != 0).sum(1)
        assert x.shape == (B, L) and ks.min() == 0 and ks.max() == L and (B <= L or sorted(set(ks.tolist())) == list(range(L + 1)))
        res, ran = scores_of(clf, x)
        assert HEAD in ran and not (ran & NOT_HERE), sorted(ran)
        refs = score_refs(sd, fe, x)
        rows = grade_rows(res.scores.cpu().numpy().astype(np.float64), res.logits.cpu().numpy().reshape(-1).astype(np.float64), refs)
        G.assert_grade(f"locus scores {layout} d{d} {mode} L{L} B{B}", rows)
        if (layout, d, mode, seed) in WITNESS_CASES and L == 9 and B == 33:
            wit = grade_rows(*witness_scores(sd, fe, x), refs)
            print("witness e/noise", [round(r.ratio, 1) for r in wit])
            assert not wit[0].ok, (wit[0].what, wit[0].ratio)


# ---- 3. exact structure -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 8, 9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", [EDGE, ("tiny", 16, "adj", 184)])
def test_structure_is_exact_and_the_logits_are_the_long_forwards_bits(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    x = scores_batch(np.random.default_rng(seed + 7 * L), N, L, 37)
    rc, scores, logits, order, ran = c_scores(clf, x, 32)
    assert rc == 0 and ran == (ran - NOT_HERE) and HEAD in ran
    real = torch.from_numpy(x != 0).cuda()
    assert not torch.isnan(scores).any() and not torch.isnan(logits).any() and not (order == -77).any()      # every element was written
    assert (scores[~real] == 0.0).all() and not torch.signbit(scores[~real]).any()                           # exactly +0.0f at padding slots
    empty = ~real.any(1)
    assert empty.any() and (scores[empty] == 0.0).all() and (logits[empty] == 0.0).all() and (order[empty] == -1).all()
    # the logit is the masked mean of the scores (float32 sum in slot order is the kernel's token order: pads add exact zeros)
    k = real.sum(1)
    assert torch.allclose(scores.double().sum(1) / (k.double() + 1e-15), logits.double(), rtol=1e-5, atol=1e-6)
    # bitwise what matcha_forward_long writes for the same (x, L)
    rc2, lg, ran2 = c_forward(clf, x, long_rows=True)
    assert rc2 == 0 and "head_fwd_kernel" in ran2 and HEAD not in ran2
    assert np.array_equal(logits.cpu().numpy().view(np.uint32), lg.astype(np.float32).view(np.uint32))
    # without the optional outputs the scores are the same bits
    rc3, scores3, _, none, _ = c_scores(clf, x, 0)
    assert rc3 == 0 and none is None and torch.equal(scores3, scores)


# ---- 4. the order -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 9, 17, 32])
def test_order_is_the_twins_rule_on_the_returned_scores(L):
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    x = scores_batch(np.random.default_rng(4000 + L), N, L, 37)
    first = None
    for lowest in sorted({1, 3, L, 32}):
        res, _ = scores_of(clf, x, lowest=lowest)
        s = res.scores.cpu().numpy()
        want = OR.lowest_order(s, x, lowest)
        assert np.array_equal(res.order.cpu().numpy(), want), (L, lowest)
        first = s if first is None else first
        assert np.array_equal(first.view(np.uint32), s.view(np.uint32))                  # `lowest` does not touch the scores


def test_order_with_every_score_equal_is_the_real_slots_ascending():
    num = synth.LAYOUTS["tiny"]
    clf, _ = hip_model(num, 16, "table", 1915)
    clf.eval()
    with torch.no_grad():
        clf.pff_classifier.PWF_Conv0.weight.zero_()
        bias = clf.pff_classifier.PWF_Conv0.bias.detach().clone().view(())
    x = scores_batch(np.random.default_rng(1915), int(np.sum(num)), 17, 33)
    res, _ = scores_of(clf, x, lowest=17)
    real = torch.from_numpy(x != 0).cuda()
    assert (res.scores[real] == bias).all() and (res.scores[~real] == 0.0).all()
    order = res.order.cpu().numpy()
    for b in range(len(x)):
        slots = np.flatnonzero(x[b])
        assert order[b, :len(slots)].tolist() == slots.tolist() and (order[b, len(slots):] == -1).all(), b


# ---- 5. the kernels, 6. model(x) unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_kernel_set_is_the_long_chain_plus_the_scores_head(layout, d, mode, seed):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    for L in (5, 12):
        x = rows_of(np.random.default_rng(seed + L), N, [L, 2, 1, 0, 3], L)
        _, ran_s = scores_of(clf, x, lowest=3)
        rc, _, ran_f = c_forward(clf, x, long_rows=True)
        assert rc == 0 and ran_s == (ran_f - {"head_fwd_kernel"}) | {HEAD}, (sorted(ran_s), sorted(ran_f))
        assert LONG_PLAN | {"attn_long_kernel"} <= ran_s and not (ran_s & NOT_HERE)


def test_model_is_unchanged_around_a_scores_call():
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(616)
    for L in (5, 12):                                            # model(x): the fused short path, the long chain
        x = rows_of(rng, N, [L, 2, 1, 0] + [int(k) for k in rng.integers(1, L + 1, size=33)], L)
        xt = torch.from_numpy(x).cuda()
        with torch.no_grad():
            before = clf(xt)
            clf.locus_scores(xt, lowest=3)
            after = clf(xt)
            assert torch.equal(before, after) and torch.equal(clf(xt, get_outlier=3), before) and before.shape == (len(x), 1)
    # ... and on ONE workspace through the C entries: forward, scores, forward
    x = rows_of(rng, N, [12, 2, 1, 0] + [int(k) for k in rng.integers(1, 13, size=33)], 12)
    rt = clf._runtime()
    ws = rt.workspace(len(x), 12, long_rows=True)
    with torch.no_grad():
        opts, _ = clf._opts(rt, False)
    opts.training, opts.forward_only, opts.status = 0, 1, rt.status.data_ptr()
    xt = torch.from_numpy(x).cuda()
    out = []
    for i in range(3):
        if i == 1:
            rc, scores, logits, _, _ = c_scores(clf, x, 3, ws=ws)
            assert rc == 0
            out.append(logits)
            continue
        lg = torch.full((len(x),), float("nan"), dtype=torch.float32, device="cuda")
        rc = rt.lib.matcha_forward_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), len(x), 12, _lib.ptr(lg),
                                        None, _lib.ptr(ws), ws.numel(), rt.stream())
        assert rc == 0
        out.append(lg)
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[0], out[1])


def test_refusals_come_before_any_launch():
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    x = rows_of(np.random.default_rng(1606), N, [9, 4, 12, 2], 12)
    with _lib.launch_log() as log:
        clf.train()
        try:
            with torch.no_grad(), pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
                clf.locus_scores(torch.from_numpy(x))
        finally:
            clf.eval()
        with torch.no_grad():
            with pytest.raises(ValueError, match="32"):
                clf.locus_scores(torch.zeros(2, 33, dtype=torch.long))
            with pytest.raises(ValueError, match="columns"):
                clf.locus_scores(torch.ones(2, 1, dtype=torch.long))
            with pytest.raises(ValueError, match="lowest"):
                clf.locus_scores(torch.from_numpy(x), lowest=33)
    assert not log.counts, log.counts
    rc, scores, logits, order, ran = c_scores(clf, x, 3, training=1)
    assert rc == -22 and not ran and torch.isnan(scores).all() and "inference-only" in _lib.load().matcha_last_error().decode()
    bad = x.copy()
    bad[2, 7] = N + 1
    with torch.no_grad():
        with pytest.raises(IndexError):
            clf.locus_scores(torch.from_numpy(bad))
        clf.locus_scores(torch.from_numpy(x))                    # the status word was cleared
        with pytest.raises(IndexError):
            with clf.deferred_id_check():
                clf.locus_scores(torch.from_numpy(bad))          # no read-back here: raised at the end of the block
                clf.locus_scores(torch.from_numpy(x))


def test_adj_mode_takes_one_draw_per_call():
    clf, sd, fe = model("tiny", 16, "adj", 184)
    num = synth.LAYOUTS["tiny"]
    x = torch.from_numpy(rows_of(np.random.default_rng(3), int(np.sum(num)), [5, 2, 9], 9))
    with torch.no_grad():
        np.random.seed(3)
        clf.locus_scores(x, lowest=2)
        after = np.random.random()
    np.random.seed(3)
    np.random.choice(np.arange(len(num)), 1)
    assert after == np.random.random()


# ---- 7. the plant -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 8, 9, 25, 32])
@pytest.mark.parametrize("layout", ["tiny", "hg38_1mb"])
def test_plant_is_the_twin_bit_for_bit(layout, L):
    """P = 37 positives x 3 draws = 111 rows (13 full blocks of eight rows and a partial one); min_dis 0 / 2, with and without the pair set,
    cycle on and off, n0 = 0 / 1000: rows, planted and the status word equal the twin's, and two chunks with matching n0 equal one call."""
    met = set()
    for min_dis in (0, 2):
        num, pos, known, known_rows, pairs, pair_rows = OR.plant_case(layout, L, min_dis)
        n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
        hset = HyperedgeSet(torch.from_numpy(known_rows).cuda())
        pset = HyperedgeSet(torch.from_numpy(pair_rows).cuda())
        post = torch.from_numpy(pos).cuda()
        for with_pairs in (False, True):
            planter = OutlierPlanter(hset, n2c, cr, pair_set=pset if with_pairs else None, min_dis=min_dis, seed=11)
            for cycle in (False, True):
                for n0 in (0, 1000):
                    with _lib.launch_log() as log:
                        rows, planted = planter.plant(post, draws=3, cycle=cycle, n0=n0)
                        status = planter.status.cpu().numpy().copy()
                    assert dict(log.counts) == {"outlier_plant_kernel": 1}, log.counts
                    planter.status.zero_()
                    w_rows, w_planted, w_status = OR.plant_outliers(pos, known, pairs if with_pairs else set(), n2c, cr, 3, cycle, min_dis, 11, n0=n0)
                    label = (layout, L, min_dis, with_pairs, cycle, n0)
                    assert rows.shape == (111, L) and planted.shape == (111,) and planted.dtype == torch.int32
                    assert np.array_equal(rows.cpu().numpy(), w_rows), label
                    assert np.array_equal(planted.cpu().numpy(), w_planted), label
                    assert status.tolist() == w_status.tolist(), (label, status, w_status)
                    met.add("exhausted" if w_status[1] else "all planted")
                    # two chunks with matching n0 equal one call (a cut at a positive: 20 positives = 60 rows)
                    a = planter.plant(post[:20], draws=3, cycle=cycle, n0=n0)
                    b = planter.plant(post[20:], draws=3, cycle=cycle, n0=n0 + 60)
                    planter.status.zero_()
                    assert torch.equal(torch.cat([a[0], b[0]]), rows) and torch.equal(torch.cat([a[1], b[1]]), planted), label
    assert "all planted" in met


def test_plant_failure_values_and_empty_sets():
    n2c = np.array([-1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.int32)
    cr = np.array([[1, 2], [2, 9]], dtype=np.int32)
    pos = np.array([[1, 4, 0], [3, 6, 0], [5, 0, 0], [0, 0, 0], [2, 9, 0], [2, 3, 8]], dtype=np.int64)
    planter = OutlierPlanter(HyperedgeSet.empty("cuda", 3), n2c, cr, min_dis=0, seed=1)
    rows, planted = planter.plant(torch.from_numpy(pos).cuda(), draws=2, cycle=True)
    w_rows, w_planted, w_status = OR.plant_outliers(pos, set(), set(), n2c, cr, 2, True, 0, 1)
    assert np.array_equal(rows.cpu().numpy(), w_rows) and np.array_equal(planted.cpu().numpy(), w_planted)
    assert planter.status.tolist() == w_status.tolist() == [OR.STATUS_BAD_CHROM, 1, 0, 0]
    with pytest.raises(KeyError):
        planter.check_status()
    assert planter.status.tolist() == [0, 0, 0, 0]
    rows, planted = planter.plant(torch.from_numpy(pos[:2]).cuda(), draws=2, cycle=True)
    assert planter.check_status() == 1 and planted.tolist()[0] == -1
    with pytest.raises(ValueError, match="32"):
        planter.plant(torch.zeros(2, 33, dtype=torch.long))


# ---- 8. the benchmark ---------------------------------------------------------------------------------------------------------------------------
def test_benchmark_counts_equal_a_recount_and_do_not_depend_on_the_chunks():
    clf, sd, fe = model(*EDGE)
    num, pos, known, known_rows, pairs, pair_rows = OR.plant_case("hg38_1mb", 25, 2, P=101)
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    hset = HyperedgeSet(torch.from_numpy(known_rows).cuda())
    pset = HyperedgeSet(torch.from_numpy(pair_rows).cuda())
    planter = OutlierPlanter(hset, n2c, cr, pair_set=pset, min_dis=2, seed=5)
    with _lib.launch_log() as log:
        one = outlier_benchmark(clf, pos, planter, top=3, draws=2, chunk_rows=1000, keep=True)
    assert log.counts.get(HEAD) == 1 and log.counts.get("outlier_plant_kernel") == 1 and "head_fwd_kernel" not in log.counts, log.counts
    many = outlier_benchmark(clf, pos, planter, top=3, draws=2, chunk_rows=16, keep=True)
    assert planter.check_status() == 2 * int((one["planted"] < 0).sum())
    assert one["planted_rows"].shape == (202, 25) and torch.equal(one["planted_rows"], many["planted_rows"]) and torch.equal(one["planted"], many["planted"])
    w_rows, w_planted, _ = OR.plant_outliers(pos, known, pairs, n2c, cr, 2, False, 2, 5)
    assert np.array_equal(one["planted_rows"].cpu().numpy(), w_rows) and np.array_equal(one["planted"].cpu().numpy(), w_planted)
    for res in (one, many):
        rows_np, planted_np, order_np = (res[k].cpu().numpy() for k in ("planted_rows", "planted", "order"))
        want = OR.hits_recount(order_np, planted_np, (rows_np != 0).sum(1), 3)
        assert sorted(res["sizes"]) == [s for s in want if want[s][0]] and res["top"] == 3
        for s, e in res["sizes"].items():
            assert e["rows"] == want[s][0] and e["hit"] == np.cumsum(want[s][1]).tolist(), (s, e, want[s])
            assert e["chance"] == [min(r, s) / s for r in (1, 2, 3)] and e["hit"][-1] <= e["rows"]
        assert res["overall"]["rows"] == sum(v[0] for v in want.values()) == int((planted_np >= 0).sum())
        assert res["overall"]["hit"] == np.cumsum(np.sum([v[1] for v in want.values()], axis=0)).tolist()
    # a chunk is scored at its own width: the chunks of 16 positives are narrower than 25 where no 25-locus row falls into them
    assert one["overall"]["rows"] == many["overall"]["rows"]


# ---- 9. the consumer ----------------------------------------------------------------------------------------------------------------------------
def test_predict_outliers_cli(tmp_path):
    import Modules  # noqa: F401
    g = gold("g6_inference_tiny.npz")
    bin2node = {str(k): int(v) for k, v in zip(g["bin_keys"], g["bin_vals"])}
    node2bin = {v: k for k, v in bin2node.items()}
    names, res = [str(n) for n in g["names"]], int(g["res"])
    N = int(np.sum(synth.LAYOUTS["tiny"]))
    rng = np.random.default_rng(1908)
    sizes = [25, 2, 9] + [int(k) for k in rng.integers(2, 26, size=20)]
    lines = [np.sort(rng.choice(N, size=k, replace=False) + 1) for k in sizes]

    def write(path, rows):
        with open(path, "w") as f:
            for r in rows:
                f.write("\t".join(node2bin[int(v)] for v in rng.permutation(r)) + "\n")

    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    np.save(os.path.join(temp, "bin2node.npy"), bin2node, allow_pickle=True)
    np.save(os.path.join(temp, "node2bin.npy"), node2bin, allow_pickle=True)
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": res, "chrom_list": names, "min_distance": 2}, f)
    inp, out, npz, multi = (os.path.join(tmp_path, n) for n in ("in.txt", "outliers.tsv", "scores.npz", "multiway.txt"))
    write(inp, lines)
    PR.main(["outliers", "-i", inp, "-o", out, "--lowest", "3", "--scores", npz, "--config", cpath])
    PR.main(["multiway", "-i", inp, "-o", multi, "--config", cpath])
    # one chunk of width 25: the long chain on both sides, the probabilities line for line
    got = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert len(got) == len(lines) and [float(r[0]) for r in got] == np.loadtxt(multi).tolist()
    z = np.load(npz)
    assert sorted(z.files) == ["offsets", "scores", "sizes"]
    assert z["sizes"].tolist() == sizes and z["offsets"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert z["scores"].shape == (z["offsets"][-1],) and z["scores"].dtype == np.float32
    clf = torch.load(os.path.join(temp, "model2load"), map_location="cuda", weights_only=False).eval()
    x = np.zeros((len(lines), 25), dtype=np.int64)
    for i, r in enumerate(lines):
        x[i, :len(r)] = r
    with torch.no_grad():
        ref = clf.locus_scores(torch.from_numpy(x), lowest=3)
    for i, k in enumerate(sizes):
        sc = z["scores"][z["offsets"][i]:z["offsets"][i + 1]]
        assert np.array_equal(sc, ref.scores[i, :k].cpu().numpy()), i
        assert int(got[i][1]) == k and len(got[i]) == 2 + 2 * min(3, k)
        for j in range(min(3, k)):
            slot = int(ref.order[i, j])
            assert got[i][2 + 2 * j] == node2bin[int(x[i, slot])] and float(got[i][3 + 2 * j]) == float(sc[slot]), (i, j)
    # chunks of 7 lines, each padded to its own longest row, against `predict`'s chunks of 7: the same lines in the same order
    small = PR.locus_scores(clf, [[int(v) for v in r] for r in lines], batch_size=7, lowest=2)
    logit7 = PR.predict(clf, [[int(v) for v in r] for r in lines], batch_size=7).reshape(-1)
    assert small["sizes"].tolist() == sizes and small["lowest"].shape == (len(lines), 2)
    assert np.abs(small["logit"] - logit7).max() <= 1e-5 * np.abs(logit7).max()
    wide = [c for c in range(0, len(lines), 7) if max(sizes[c:c + 7]) > 8]
    for c in wide:                                               # a chunk wider than 8 runs the same chain on both sides: the same bits
        assert np.array_equal(small["logit"][c:c + 7], logit7[c:c + 7]), c
    assert wide
    # a 33-bin line is refused by its number before anything is scored
    write(inp, lines[:10] + [np.arange(1, 34)] + lines[10:])
    os.remove(out)
    with pytest.raises(ValueError, match=r"line 11 has 33 distinct bins"):
        PR.main(["outliers", "-i", inp, "-o", out, "--config", cpath])
    assert not os.path.exists(out)
