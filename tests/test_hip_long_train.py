"""Training on rows of 9 to 32 nodes on the device (Classifier.long_row_training; matcha_forward_long_train / matcha_backward_long;
attn_long_bwd_kernel): the attention backward alone against torch fp64 autograd, parity with the real reference's step
(tests/golden/g13_long_grads.npz), the fp32 grade of the whole step (tests/fp64_grade.py as it is, K = 8) without and with dropout, the long
entry points beside the L <= 8 ones on identical input, shape edges, ten AdamW steps, and the surface.  GPU only (-m gpu)."""
import ctypes as C
import io
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from matcha_amd import _lib, synth
from tests import fp64_grade as G
from tests.helpers import GOLD, gold, logit_err, oracle_state, rel_err
from tests.test_cpu_long_train import GRADE_CASES, golden_sd, grade_case, predraw_chrom, rows_of
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
BETA = 0.001
LONG_PLAN = {"long_plan_count_kernel", "long_plan_scan_kernel", "long_plan_fill_kernel"}
LONG_TRAIN = LONG_PLAN | {"attn_long_kernel", "attn_long_bwd_kernel"}
SHORT_BWD = {"attn_bwd_kernel", "fused_bwdh_kernel", "enc128_bwd_kernel"}

_MODELS = {}


def model(layout, d, mode, seed, dropout=False):
    """(clf in train mode with long_row_training on, sd, fe): one model per configuration for the whole module; dropout off unless asked."""
    key = (layout, d, mode, seed, dropout)
    if key not in _MODELS:
        num = synth.LAYOUTS[layout]
        _, fe, sd = oracle_state(num, d, mode, seed)
        clf, _ = hip_model(num, d, mode, seed, sd=sd)
        if not dropout:
            for m in clf.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
        clf.long_row_training = True
        _MODELS[key] = (clf.train(), sd, fe)
    return _MODELS[key]


def step(clf, x, y, w, np_seed=None):
    """One loss.backward() of loss = bce + 0.001 recon through model(x): (StepOut, kernels that ran)."""
    for p in clf.parameters():
        p.grad = None
    if np_seed is not None:
        np.random.seed(np_seed)
    xd = torch.from_numpy(x).cuda()
    yd, wd = torch.from_numpy(y).cuda().view(-1, 1), torch.from_numpy(w).cuda().view(-1, 1)
    with _lib.launch_log() as log:
        logits, recon = clf(xd, return_recon=True)
        bce = F.binary_cross_entropy_with_logits(logits, yd, weight=wd)
        (bce * 1.0 + recon * BETA).backward()
        torch.cuda.synchronize()
    assert logits.shape == (len(x), 1)
    grads = {n: (None if p.grad is None else p.grad.detach().cpu().double().numpy()) for n, p in clf.named_parameters()}
    out = G.StepOut(logits.detach().cpu().double().numpy().reshape(-1), {"bce": float(bce), "recon": float(recon.reshape(-1)[0])}, grads)
    return out, {k for k, n in log.counts.items() if n > 0}


def assert_parity(label, got, ref, tol=TOL):
    """logits by logit_err, every gradient by rel_err, equal None sets -- against a StepOut-like reference."""
    e = logit_err(got.logits, ref.logits)
    none_got = {n for n, v in got.grads.items() if v is None} - G.FROZEN_NAMES
    none_ref = {n for n, v in ref.grads.items() if v is None} - G.FROZEN_NAMES
    assert none_got == none_ref, (label, sorted(none_got ^ none_ref))
    worst = ("", 0.0)
    for n, v in ref.grads.items():
        if v is None or n == G.GAUGE or n in G.FROZEN_NAMES:
            continue
        r = rel_err(got.grads[n], v)
        if r > worst[1]:
            worst = (n, r)
    print(f"{label}: logit_err {e:.2e}, worst gradient rel_err {worst[1]:.2e} ({worst[0]})")
    assert e <= tol, (label, e)
    assert worst[1] <= tol, (label, worst)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------------
def torch_attention(Q, K, V, row_off, L, d, shared):
    """O [T + 1, 8 d] of the long rows' attention in torch (any dtype): only the diagonal masked, the n_pad = L - k padding slots one extra key
    column (the shared padding token's row T) with multiplicity n_pad; padding queries are not evaluated (their O rows stay 0)."""
    T = int(row_off[-1])
    rows = []
    for b in range(len(row_off) - 1):
        t0, k = int(row_off[b]), int(row_off[b + 1] - row_off[b])
        if k == 0:
            continue
        n_pad = L - k
        heads = []
        for h in range(8):
            q = Q[t0:t0 + k, h * d:(h + 1) * d]
            kk = K[:, :d] if shared else K[:, h * d:(h + 1) * d]
            vv = V[:, :d] if shared else V[:, h * d:(h + 1) * d]
            keys, vals = kk[t0:t0 + k], vv[t0:t0 + k]
            s = q @ keys.t() / np.sqrt(d)
            s = s.masked_fill(torch.eye(k, dtype=torch.bool), float("-inf"))
            if n_pad > 0:
                sp = q @ kk[T] / np.sqrt(d) + np.log(n_pad)
                s, vals = torch.cat([s, sp[:, None]], 1), torch.cat([vals, vv[T:T + 1]], 0)
            heads.append(torch.softmax(s, 1) @ vals)
        rows.append((t0, torch.cat(heads, 1)))
    O = torch.zeros(T + 1, 8 * d, dtype=Q.dtype)
    return O, rows


def torch_attention_grads(Qn, Kn, Vn, dOn, row_off, L, d, shared, dtype):
    Q, K, V = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (Qn, Kn, Vn))
    dO = torch.from_numpy(dOn).to(dtype)
    _, rows = torch_attention(Q, K, V, row_off, L, d, shared)
    loss = sum((o * dO[t0:t0 + len(o)]).sum() for t0, o in rows)
    return [g.double().numpy() for g in torch.autograd.grad(loss, [Q, K, V])]


@pytest.mark.parametrize("L", [9, 32])
@pytest.mark.parametrize("d,shared", [(16, False), (64, True), (128, True)])
def test_attention_backward_kernel_against_torch_fp64(d, shared, L):
    attention_backward_case(d, shared, L, [L, 2, 1, 0, 9, L - 1, 17 if L == 32 else 5], 1000 + d + L)


def attention_backward_case(d, shared, L, ks, seed, q_scale=1.0, pad_row=False, reference=None):
    """matcha_attn_long_bwd on hyperedges of ks real tokens against torch fp64 autograd, e <= 8 x torch fp32's own error per tensor, twice over NaN
    and 7.0 fills with equal bits; ``q_scale`` multiplies Q (sharp scores); with ``pad_row`` the padding token's dK / dV row is held to the same
    bound on its own, normalised by that row's fp64 maximum; ``reference`` stands in for torch_attention_grads (same signature).  Returns {tensor: e / noise} (and "dK pad" / "dV pad")."""
    lib = _lib.load()
    row_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    T, B = int(row_off[-1]), len(ks)
    rng = np.random.default_rng(seed)
    kvw = d if shared else 8 * d
    Qn, dOn = (rng.standard_normal((T + 1, 8 * d)).astype(np.float32) for _ in range(2))
    Kn, Vn = (rng.standard_normal((T + 1, kvw)).astype(np.float32) for _ in range(2))
    if q_scale != 1.0:
        Qn = (Qn * np.float32(q_scale)).astype(np.float32)
    dOn[T] = 0.0                                             # the padding token is no query: its dO row is the masked fc1 row's gradient, zero
    reference = reference or torch_attention_grads
    r64 = reference(Qn, Kn, Vn, dOn, row_off, L, d, shared, torch.float64)
    r32 = reference(Qn, Kn, Vn, dOn, row_off, L, d, shared, torch.float32)
    dev = lambda a: torch.from_numpy(a).cuda().contiguous()
    Q, K, V, dO, ro = dev(Qn), dev(Kn), dev(Vn), dev(dOn), dev(row_off)
    ws = torch.empty(lib.matcha_attn_long_bwd_workspace_bytes(B, d), dtype=torch.uint8, device="cuda")
    runs = []
    for fill in (float("nan"), 7.0):                         # every output row is written, whatever the buffers held
        dQ, dK, dV = torch.full_like(Q, fill), torch.full_like(K, fill), torch.full_like(V, fill)
        ws.fill_(0xFF)
        with _lib.launch_log() as log:
            rc = lib.matcha_attn_long_bwd(_lib.ptr(Q), _lib.ptr(K), _lib.ptr(V), _lib.ptr(dO), _lib.ptr(ro), B, L, d, int(shared), _lib.ptr(dQ), _lib.ptr(dK),
                                          _lib.ptr(dV), _lib.ptr(ws), ws.numel(), None)
            torch.cuda.synchronize()
        assert rc == 0, lib.matcha_last_error().decode()
        assert log.counts.get("attn_long_bwd_kernel") == 1
        runs.append([t.cpu().numpy() for t in (dQ, dK, dV)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                          # bit-identical from run to run
    ratios = {}
    for name, got, g64, g32 in zip(("dQ", "dK", "dV"), runs[0], r64, r32):
        e, noise = G.tensor_err(got, g64), max(G.tensor_err(g32, g64), G.ULP)
        e_pad = float(np.abs(got[T] - g64[T]).max() / max(np.abs(g64).max(), 1e-300))
        print(f"d {d} L {L} {name}: e {e:.2e}, torch fp32 {noise:.2e}, ratio {e / noise:.2f}; padding row e {e_pad:.2e}")
        assert np.isfinite(got).all()
        assert e <= 8 * noise, (name, e, noise)
        ratios[name] = e / noise
        if pad_row and name != "dQ":
            e_row, noise_row = G.tensor_err(got[T], g64[T]), max(G.tensor_err(g32[T], g64[T]), G.ULP)
            print(f"d {d} L {L} {name}: padding row alone e {e_row:.2e}, torch fp32 {noise_row:.2e}, ratio {e_row / noise_row:.2f}")
            assert e_row <= 8 * noise_row, (name, "padding row", e_row, noise_row)
            ratios[name + " pad"] = e_row / noise_row
    assert not runs[0][0][T].any()                           # dQ of the padding token
    return ratios


# ---- 2. reference parity ------------------------------------------------------------------------------------------------------------------------
class _Ref:
    def __init__(self, g, tag):
        self.logits = g[f"logits_{tag}"]
        self.grads = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(f"grad_{tag}/")}
        self.grads.update({n: None for n in g[f"none_{tag}"].tolist()})


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_reference_parity_of_the_long_training_step(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    g = gold("g13_long_grads.npz")
    clf = torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False)
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    clf.train()
    clf.long_row_training = True
    C_ = len(synth.LAYOUTS["tiny"])
    for L in (9, 32):
        tag = f"{mode}_L{L}"
        assert predraw_chrom(C_, 4300 + L) == int(g[f"chrom_{tag}"])
        got, ran = step(clf, g[f"x_L{L}"].astype(np.int64), g[f"y_L{L}"].reshape(-1), g[f"w_L{L}"].reshape(-1), np_seed=4300 + L)
        assert_parity(f"reference {tag}", got, _Ref(g, tag))
        assert abs(got.losses["bce"] - float(g[f"bce_{tag}"])) <= TOL * max(1.0, abs(float(g[f"bce_{tag}"])))
        assert abs(got.losses["recon"] - float(g[f"recon_{tag}"])) <= TOL * max(1.0, abs(float(g[f"recon_{tag}"])))
        assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), sorted(ran)


# ---- 3. fp32 grade of the whole step, dropout off ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_long_training_step_at_fp32_grade(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    x, y, w, chrom = grade_case(layout, d, mode, seed, L)
    ref = G.references(sd, fe, x, y, w, chrom=chrom, beta=BETA)
    got, ran = step(clf, x, y, w, np_seed=seed + L)
    assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), sorted(ran)
    assert got.logits[3] == 0.0                                               # the all-padding row
    G.assert_grade(f"long step {layout} d{d} {mode} L{L}", G.grade(got, ref))


# ---- 4. fp32 grade with dropout on --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,mode,seed", [GRADE_CASES[0], GRADE_CASES[3]])
def test_long_training_step_with_dropout_at_fp32_grade(layout, d, mode, seed):
    L = 17
    clf, sd, fe = model(layout, d, mode, seed, dropout=True)
    ps = clf._dropout_p()
    assert ps[1] > 0 and ps[2] > 0 and clf.training
    x, y, w, chrom = grade_case(layout, d, mode, seed, L)
    rt = clf._runtime()
    call_seed = (int(torch.initial_seed()) * 1000003 + rt.seed_counter + 1) & 0x7FFFFFFFFFFFFFFF
    masks = G.step_masks(call_seed, ps, x.size, d, synth.LAYOUTS[layout] if mode == "adj" else None)
    ref = G.references(sd, fe, x, y, w, chrom=chrom, beta=BETA, masks=masks)
    got, ran = step(clf, x, y, w, np_seed=seed + L)
    assert clf._runtime() is rt and rt.seed_counter >= 1
    assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), sorted(ran)
    G.assert_grade(f"long step, dropout, {layout} d{d} {mode} L{L}", G.grade(got, ref))
    ref0 = G.oracle_step(sd, fe, x, y, w, chrom=chrom, beta=BETA, backward=False)
    assert logit_err(got.logits, ref0.logits) > 100 * TOL                     # (and the masks did something)


# ---- 5. long against short on identical input -------------------------------------------------------------------------------------------------------
def c_step(clf, x, y, w, chrom, long_rows):
    """The two entry points called directly (forward, then backward with dlogits of the weighted BCE mean and drecon = BETA): (StepOut, kernels)."""
    rt = clf._runtime()
    lib = rt.lib
    np.random.seed(0)
    opts, _ = clf._opts(rt, True)
    opts.training, opts.forward_only, opts.random_chrom = 1, 0, chrom
    opts.status = rt.status.data_ptr()
    xt = torch.from_numpy(x).cuda().contiguous()
    B, L = xt.shape
    ws = rt.workspace(B, L, long_train=True) if long_rows else rt.workspace(B, L)
    logits = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    losses = torch.zeros(3, dtype=torch.float32, device="cuda")
    gflat = torch.zeros(rt.n_flat, dtype=torch.float32, device="cuda")
    grads = rt.tensors_for(gflat)
    touched = torch.zeros(rt.n_touched, dtype=torch.int32, device="cuda")
    head = (C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), B, L)
    with _lib.launch_log() as log:
        if long_rows:
            rc = lib.matcha_forward_long_train(*head, _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream())
        else:
            rc = lib.matcha_forward(*head, None, None, _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream())
        assert rc == 0, lib.matcha_last_error().decode()
        dl = (torch.from_numpy(w).cuda() * (torch.sigmoid(logits) - torch.from_numpy(y).cuda()) / B).contiguous()
        dr = torch.full((1,), BETA, dtype=torch.float32, device="cuda")
        tail = (C.byref(grads), _lib.ptr(touched), _lib.ptr(ws), ws.numel(), rt.stream())
        if long_rows:
            rc = lib.matcha_backward_long(*head, _lib.ptr(dl), _lib.ptr(dr), *tail)
            again = lib.matcha_backward_long(*head, _lib.ptr(dl), _lib.ptr(dr), *tail)       # one backward per forward
            assert again == -22 and "on record" in lib.matcha_last_error().decode()
        else:
            rc = lib.matcha_backward(*head, None, None, _lib.ptr(dl), _lib.ptr(dr), *tail)
        assert rc == 0, lib.matcha_last_error().decode()
        torch.cuda.synchronize()
    names = {id(p): n for n, p in clf.named_parameters()}
    tl = touched.tolist()
    out = {n: None for n, _ in clf.named_parameters()}
    for p, o, grp in zip(rt.live, rt.seg_off_list[:-1], rt.seg_group_list):
        if rt.mode == 0 or grp < 2 or tl[grp]:
            out[names[id(p)]] = gflat[o:o + p.numel()].view(p.shape).cpu().double().numpy()
    return G.StepOut(logits.cpu().double().numpy(), {}, out), {k for k, n in log.counts.items() if n > 0}


@pytest.mark.parametrize("layout,d,mode,seed", [GRADE_CASES[0], GRADE_CASES[3]])
@pytest.mark.parametrize("L", [8, 5])
def test_long_entry_points_against_the_short_ones(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    N = int(np.sum(synth.LAYOUTS[layout]))
    rng = np.random.default_rng(seed + 40 + L)
    ks = [L, 2, 1, 0] + [int(k) for k in rng.integers(0, L + 1, size=253)]
    x = rows_of(rng, N, ks, L)
    y, w = (rng.random(257) < 0.5).astype(np.float32), (0.5 + 1.5 * rng.random(257)).astype(np.float32)
    ref = G.references(sd, fe, x, y, w, chrom=1, beta=BETA)
    got_l, ran_l = c_step(clf, x, y, w, 1, True)
    got_s, ran_s = c_step(clf, x, y, w, 1, False)
    assert LONG_TRAIN <= ran_l and not (ran_l & SHORT_BWD) and not (ran_s & LONG_TRAIN), (sorted(ran_l), sorted(ran_s))
    G.assert_grade(f"long entry points {layout} d{d} L{L}", G.grade(got_l, ref))
    G.assert_grade(f"short entry points {layout} d{d} L{L}", G.grade(got_s, ref))


# ---- 6. shapes, each against the fp32 oracle at TOL -----------------------------------------------------------------------------------------------
EDGE = GRADE_CASES[0]


def _against_oracle(label, x, seed=0):
    clf, sd, fe = model(*EDGE)
    rng = np.random.default_rng(600 + seed)
    y, w = (rng.random(len(x)) < 0.5).astype(np.float32), (0.5 + 1.5 * rng.random(len(x))).astype(np.float32)
    got, ran = step(clf, x, y, w)
    assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), sorted(ran)
    assert_parity(label, got, G.oracle_step(sd, fe, x, y, w, beta=BETA))
    return got


@pytest.mark.parametrize("B", [1, 3, 257])
def test_train_batch_sizes_at_width_17(B):
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(400 + B)
    ks = ([17] + [int(k) for k in rng.integers(1, 18, size=B - 1)])[:B]
    _against_oracle(f"B {B} L 17", rows_of(rng, N, ks, 17), B)


def test_train_on_a_batch_of_empty_rows():
    clf, sd, fe = model(*EDGE)
    x = np.zeros((5, 17), dtype=np.int64)
    got, ran = step(clf, x, np.ones(5, dtype=np.float32), np.ones(5, dtype=np.float32))
    assert LONG_TRAIN <= ran
    assert not got.logits.any()
    for n, v in got.grads.items():
        assert v is None or not v.any(), n


def test_train_pads_inside_rows_repeated_ids_and_empty_runs():
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(617)
    L, B = 17, 300
    ks = [int(k) for k in rng.integers(1, L + 1, size=B)]
    x = rows_of(rng, N, ks, L)
    for b in range(0, B, 3):                                  # pads anywhere in the row: the real ids keep their order, the slots move
        slots = np.sort(rng.choice(L, size=ks[b], replace=False))
        row = np.zeros(L, dtype=np.int64)
        row[slots] = x[b, :ks[b]]
        x[b] = row
    x[1, :4] = [7, 9, 9, 30]                                  # one id twice in a row: its table gradient row gets both contributions
    x[4, :L] = np.sort(rng.choice(N, size=L, replace=False) + 1)
    x[4, 5] = x[4, 11]
    x[100:170] = 0                                            # a run of 70 empty rows
    got = _against_oracle("pads inside rows, repeated ids, empty run", x, 17)
    assert not got.logits[100:170].any()


def test_train_full_rows_513_by_32():
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(632)
    x = np.sort(np.argsort(rng.random((513, N)), axis=1)[:, :32] + 1, axis=1).astype(np.int64)
    _against_oracle("B 513 L 32 k 32", x, 32)


def test_train_one_long_row_among_short_ones():
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(625)
    ks = [3] * 513
    ks[300] = 25
    _against_oracle("B 513 L 25, one row of 25", rows_of(rng, N, ks, 25), 25)


# ---- 7. ten AdamW steps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_ten_adamw_steps_match_the_oracle(mode):
    """lr 1e-3, torch.optim.AdamW defaults (main.py:630), on the model and on the oracle's parameters; same batch, same chromosome draws."""
    from oracle import hypersagnn as O
    num = synth.LAYOUTS["tiny"]
    _, fe, sd = oracle_state(num, 16, mode, 77)
    clf, _ = hip_model(num, 16, mode, 77, sd=sd)
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    clf.train()
    clf.long_row_training = True
    rng = np.random.default_rng(712)
    x = rows_of(rng, int(np.sum(num)), [12, 2, 1, 9] + [int(k) for k in rng.integers(2, 13, size=44)], 12)
    y, w = (rng.random((48, 1)) < 0.5).astype(np.float32), (0.5 + 1.5 * rng.random((48, 1))).astype(np.float32)
    P = {k: torch.from_numpy(np.array(v)).requires_grad_(k not in G.FROZEN_NAMES) for k, v in sd.items()}
    names = [n for n, t in P.items() if t.requires_grad]
    opt_o = torch.optim.AdamW([P[n] for n in names], lr=1e-3)
    opt_m = torch.optim.AdamW(list(clf.parameters()), lr=1e-3)
    np.random.seed(77)
    chroms = [int(np.random.choice(np.arange(len(num)), 1)[0]) for _ in range(10)]
    np.random.seed(77)
    xd, yd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    for it in range(10):
        lg, rc = O.classifier_forward(P, fe, torch.from_numpy(x), random_chrom=chroms[it])
        opt_o.zero_grad()
        (O.bce_with_logits(lg, torch.from_numpy(y), torch.from_numpy(w)) + rc * BETA).backward()
        opt_o.step()
        logits, recon = clf(xd, return_recon=True)
        opt_m.zero_grad()
        (F.binary_cross_entropy_with_logits(logits, yd, weight=wd) + recon * BETA).backward()
        opt_m.step()
        if it in (0, 9):
            mine = dict(clf.named_parameters())
            worst = ("", 0.0)
            for n in names:
                if n == G.GAUGE:
                    continue
                r = rel_err(mine[n].detach().cpu().numpy(), P[n].detach().numpy())
                if r > worst[1]:
                    worst = (n, r)
            print(f"{mode} after step {it + 1}: worst parameter rel_err {worst[1]:.2e} ({worst[0]})")
            assert worst[1] <= TOL, (it, worst)


# ---- 8. the surface -------------------------------------------------------------------------------------------------------------------------------
def test_surface_of_the_switch():
    clf, sd, fe = model(*EDGE)
    N = int(np.sum(synth.LAYOUTS[EDGE[0]]))
    rng = np.random.default_rng(808)
    x9 = torch.from_numpy(rows_of(rng, N, [9, 3, 5, 2], 9))
    try:
        clf.long_row_training = False
        with _lib.launch_log() as log:
            with torch.no_grad(), pytest.raises(NotImplementedError, match="inference-only"):
                clf(x9)                                       # train mode
            clf.eval()
            with pytest.raises(NotImplementedError, match="inference-only"):
                clf(x9)                                       # grad enabled, trainable parameters
        assert not log.counts, log.counts
    finally:
        del clf.long_row_training                             # back to the class attribute ...
        clf.long_row_training = True                          # ... and on again
        clf.train()
    lg = clf(x9)
    lg.sum().backward()
    with pytest.raises(RuntimeError, match="second backward"):
        lg.sum().backward()
    bad = x9.clone()
    bad[2, 1] = N + 1
    with pytest.raises(IndexError):
        clf(bad)
    clf(x9)                                                   # the status word was cleared
    with pytest.raises(ValueError, match="32"):
        clf(torch.zeros(2, 33, dtype=torch.long))
    clf.eval()
    try:
        with torch.no_grad(), _lib.launch_log() as log:
            clf(x9)
            torch.cuda.synchronize()
        ran = {k for k, n in log.counts.items() if n > 0}
        assert "attn_long_kernel" in ran and "attn_long_bwd_kernel" not in ran and not (ran & SHORT_BWD), sorted(ran)
    finally:
        clf.train()
    # L = 8: the same kernels with the switch on and off
    x8, y8, w8 = G.make_case_batch(EDGE[0], [2, 5, 8], 16, 809, 8)
    sets = []
    for on in (True, False):
        clf.long_row_training = on
        _, ran = step(clf, x8, y8, w8)
        sets.append(ran)
    clf.long_row_training = True
    assert sets[0] == sets[1] and not (sets[0] & LONG_TRAIN), (sorted(sets[0]), sorted(sets[1]))
    # a model round-tripped through pickle keeps working (and keeps the switch: it is an instance attribute here)
    clf2 = pickle.loads(pickle.dumps(clf))
    assert clf2.long_row_training is True
    a, _ = step(clf, x9.numpy(), np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    b, ran = step(clf2, x9.numpy(), np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    assert LONG_TRAIN <= ran and np.array_equal(a.logits, b.logits)
