"""adj front end (MultipleEmbedding: the mode the reference's main.py runs) at feature blocks wider than 256 bins and at the largest
number of chromosomes the library takes, against the in-test oracle.  GPU only (-m gpu).

The adj kernels change shape where these layouts go: the fused embed_dim-64 backward and reconstruction kernels walk the columns in
groups of 256 (four 64-column chunks), the gather-GEMMs contract in chunks of 64 with odd-width tails, adj_tn_kernel<1> tiles W0 by 64
columns, and the counting sort in front of them changes kernels with the token count (one workgroup up to 4 096 slots; hist + scan +
scatter above, the scan without its LDS staging above 12 288 histogram entries) and sizes its LDS by the number of chromosomes."""
import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from oracle import hypersagnn as O
from oracle import rng as R
from tests.helpers import oracle_state, logit_err
from tests.test_hip_model import GAUGE, TOL, hip_model, _trainer_grads

pytestmark = pytest.mark.gpu

WIDE = synth.LAYOUTS["wide_adj"]          # [255, 256, 320, 257, 513, 2491, 64]
SORT_SMALL = {"adj_sort_small_kernel"}
SORT_LARGE = {"adj_hist_kernel", "adj_scan_kernel", "adj_scatter_kernel"}
FUSED_ADJ = {"adj_fused_fwd_kernel", "adj_recon_kernel", "adj_fused_bwd_kernel"}
LAYERWISE_ADJ = {"adj_encode_fwd_kernel", "adj_tn_kernel<1>", "adj_recon_loss_kernel"}
# variant -> (embed_dim, disable_fused, adj kernels that must run, adj kernels that must not)
VARIANTS = {
    "d64_fused": (64, 0, FUSED_ADJ, LAYERWISE_ADJ),
    "d64_unfused": (64, 2, LAYERWISE_ADJ, FUSED_ADJ),        # the layer-by-layer adj kernels at embed_dim 64 (encoder still fused)
    "d128": (128, 0, LAYERWISE_ADJ | {"enc128_fwd_kernel"}, FUSED_ADJ),
    "d32": (32, 0, LAYERWISE_ADJ, FUSED_ADJ),                # adj_encode_fwd_kernel<1>
    "d256": (256, 0, LAYERWISE_ADJ, FUSED_ADJ),              # adj_encode_fwd_kernel<8>
}
# rows per k in {2..5}, padded to L = 5: 2 048 rows = 10 240 token slots (hist / scan / scatter), 800 rows = 4 000 (adj_sort_small_kernel)
SIZES = {"large": (512, SORT_LARGE, SORT_SMALL), "small": (200, SORT_SMALL, SORT_LARGE)}
CASES = ([(v, s, c) for v in ("d64_fused", "d128") for s in SIZES for c in range(len(WIDE))]
         + [(v, s, 5) for v in ("d64_unfused", "d32", "d256") for s in SIZES])          # chromosome 5: the 2 491-bin block


def _mixed_batch(N, rows_per_k, seed, ks=(2, 3, 4, 5)):
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, rows_per_k), ((0, 0), (0, 5 - k))) for k in ks])
    x = x[rng.permutation(len(x))]
    y = (rng.random((len(x), 1)) < 0.25).astype(np.float32)
    w = np.where(y > 0, rng.uniform(0.5, 4.0, size=y.shape), 1.0).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(w)


def _chunk_err(got, ref, axis, floor=1e-2):
    """Worst error of 64-wide chunks along `axis` (columns of tied weight_0 [d, n_c], rows of the recon head [n_r, d] / its bias), each
    scaled by the chunk's OWN max |ref| -- floored at `floor` x the tensor's max -- so that an error confined to a tail chunk or to a
    second 256-column group is not measured against the block's largest element.  Returns (error, index of the worst chunk)."""
    got = np.moveaxis(np.asarray(got, dtype=np.float64), axis, 0)
    ref = np.moveaxis(np.asarray(ref, dtype=np.float64), axis, 0)
    top = np.abs(ref).max()
    worst, at = 0.0, -1
    for k0 in range(0, ref.shape[0], 64):
        r, g = ref[k0:k0 + 64], got[k0:k0 + 64]
        e = float(np.abs(g - r).max() / max(float(np.abs(r).max()), floor * top, 1e-30))
        if e > worst:
            worst, at = e, k0 // 64
    return worst, at


def _check_grads(mine, grads, num, r_chrom, tag):
    """Every gradient tensor norm-wise at TOL, the grad-None set equal to the oracle's, and per 64-column / 64-row chunk the adj tensors
    of every chromosome (tied weight_0) and the reconstruction head of chromosome r.  Returns the worst (norm-wise, per-chunk) errors."""
    # (attribute_dict_embedding.weight is frozen: the oracle does not differentiate it)
    assert {n for n, v in mine.items() if v is None} - {"attribute_dict_embedding.weight"} == {n for n, v in grads.items() if v is None}, tag
    worst, worst_chunk, n_checked = 0.0, 0.0, 0
    for n, gref in grads.items():
        if gref is None or n == GAUGE:
            continue
        r = gref.numpy()
        e = float(np.abs(mine[n].cpu().numpy() - r).max()) / max(float(np.abs(r).max()), 1e-3)
        assert e <= TOL, (tag, n, e)
        worst = max(worst, e)
        n_checked += 1
    assert n_checked >= 26, n_checked
    chunked = [(f"node_embedding.Embedding_Linear{c}.tied weight_0", 1) for c in range(len(num))]
    chunked += [(f"node_embedding.Embedding_recon{r_chrom}.FF_Linear0.weight", 0), (f"node_embedding.Embedding_recon{r_chrom}.FF_Linear0.bias", 0)]
    for n, axis in chunked:
        if grads[n] is None:                  # a chromosome without tokens in the batch (the grad-None sets agree)
            continue
        e, at = _chunk_err(mine[n].cpu().numpy(), grads[n].numpy(), axis)
        assert e <= TOL, (tag, n, "64-chunk", at, e)
        worst_chunk = max(worst_chunk, e)
    return worst, worst_chunk


def _assert_kernels(ran, must, must_not, tag):
    assert must <= ran, (tag, sorted(must - ran), sorted(ran))
    assert not (must_not & ran), (tag, sorted(must_not & ran))


@pytest.mark.parametrize("variant,size,r_chrom", CASES)
def test_trainer_step_vs_oracle_wide_blocks_dropout(variant, size, r_chrom):
    """A Trainer step (the bench's configuration: loss inside the forward, fused backward where the library fuses) with dropout ON on
    blocks of 255 / 256 / 320 / 257 / 513 / 2 491 / 64 bins against the oracle with the kernels' own masks injected (oracle/rng.py; the
    adj mask is max(num) = 2 491 columns wide, so the column counters of every 256-group are drawn).  The reconstruction chromosome is
    each of the seven blocks in turn at embed_dim 64 (fused) and 128, the 2 491-bin block for the other variants.  Logits element-wise, both losses, the grad-None set, every gradient norm-wise -- and per 64-column chunk
    tied weight_0 of every chromosome and per 64-row chunk the recon head: a wrong tail chunk or second column group must fail here."""
    from matcha_amd.engine import Trainer
    d, disable_fused, must, must_not = VARIANTS[variant]
    rows_per_k, sort_must, sort_not = SIZES[size]
    num = WIDE
    N = int(np.sum(num))
    xt, yt, wt = _mixed_batch(N, rows_per_k, 11 + r_chrom)
    with _lib.option("disable_fused", disable_fused):
        clf, _ = hip_model(num, d, "adj", 17)
        clf.train()
        base_seed, alpha, beta = 4242 + r_chrom, 1.0, 0.05
        tr = Trainer(clf, base_seed=base_seed)
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xt.cuda(), yt.cuda().reshape(-1), wt.cuda().reshape(-1), alpha, beta, r_chrom)
            torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    tag = f"{variant}/{size}/chrom {r_chrom}"
    _assert_kernels(ran, must | sort_must, must_not | sort_not, tag)
    P, fe, _ = oracle_state(num, d, "adj", 17, requires_grad=True)
    seed = base_seed + 1                       # Trainer advances the device seed before every step
    T = xt.numel()
    masks = {"fc1": torch.from_numpy(R.dropout_mask(seed, R.STREAM_DROP_FC1, O.P_DROP_FC1, T, d)),
             "pff": torch.from_numpy(R.dropout_mask(seed, R.STREAM_DROP_PFF, O.P_DROP_PFF, T, d)),
             "adj": torch.from_numpy(R.dropout_mask(seed, R.STREAM_DROP_ADJ, O.P_DROP_ADJ, T, max(num)))}
    _, bce, recon, ref_logits, grads = O.loss_and_grads(P, fe, xt, yt, wt, alpha, beta, random_chrom=r_chrom, masks=masks)
    e_logit = logit_err(logits.cpu().numpy(), ref_logits.numpy())
    assert e_logit < TOL, (tag, e_logit)
    assert abs(float(tr.losses[0]) - float(bce)) <= TOL * max(1.0, abs(float(bce))), tag
    assert abs(float(tr.losses[1]) - float(recon[0])) <= TOL * max(1.0, abs(float(recon[0]))), tag
    worst, worst_chunk = _check_grads(_trainer_grads(tr, clf), grads, num, r_chrom, tag)
    print(f"adj wide {tag}: logits {e_logit:.1e}, worst gradient {worst:.1e}, worst 64-chunk {worst_chunk:.1e}; "
          f"adj kernels {sorted(k for k in ran if k.startswith('adj_'))}")


# ---- the sort at kMaxChrom = 63 chromosomes (n_attr = 64: attr_mode 1's bound) ----------------------------------------------------------
def _layout63():
    num = [3 + (7 * i) % 61 for i in range(63)]              # widths 3 .. 63
    num[10], num[20], num[30], num[50] = 257, 700, 513, 320  # a few blocks over 256 bins: N = 3 705
    return num


# size -> (rows per k, k, sort kernels that must run, must not)
C63_SIZES = {"small": (200, (2, 3, 4, 5), SORT_SMALL, SORT_LARGE),   # 4 000 token slots: adj_sort_small_kernel, (C + 1) x 512 ints = 128 KB of LDS
             "large": (40960, (5,), SORT_LARGE, SORT_SMALL)}         # 40 960 rows of k = 5 = 204 800 tokens: 200 sort blocks x 64 buckets > 12 288
                                                                     # -> the scan's unstaged path; adj_scatter_kernel with (C + 1) x 256 ints = 64 KB


@pytest.mark.parametrize("size", sorted(C63_SIZES))
def test_adj_63_chromosomes_vs_oracle(size):
    """63 chromosomes (the library's kMaxChrom) at embed_dim 64: eval logits + reconstruction loss, then one dropout-free training step's
    loss and gradients, against the oracle -- at <= 4 096 token slots (the one-workgroup sort) and at 204 800 (hist / unstaged scan /
    scatter).  The launch log asserts which sort ran."""
    from matcha_amd.engine import Trainer
    num = _layout63()
    C, N = len(num), int(np.sum(num))
    rows_per_k, ks, sort_must, sort_not = C63_SIZES[size]
    xt, yt, wt = _mixed_batch(N, rows_per_k, 63, ks)
    if size == "large":                                      # 1 024 token slots per sort block (kSortTok), 12 288 staged histogram entries
        assert -(-xt.numel() // 1024) * (C + 1) > 12288 and int((xt != 0).sum()) > 196608
    r_chrom = 30 if size == "small" else 10                  # 513 / 257 bins (the large batch keeps the oracle's [m, n_r] residual small)
    clf, _ = hip_model(num, 64, "adj", 19)
    P, fe, _ = oracle_state(num, 64, "adj", 19, requires_grad=True)
    # eval forward: Classifier.forward draws the chromosome from numpy's global stream (Modules.py:192)
    np.random.seed(5)
    chrom_eval = int(np.random.choice(np.arange(C), 1)[0])
    clf.eval()
    np.random.seed(5)
    with _lib.launch_log() as log, torch.no_grad():
        lg, rc = clf(xt, return_recon=True)
        torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    _assert_kernels(ran, sort_must, sort_not, f"eval/{size}")
    with torch.no_grad():
        lg_ref, rc_ref = O.classifier_forward(P, fe, xt, random_chrom=chrom_eval)
    e_eval = logit_err(lg.cpu().numpy(), lg_ref.numpy())
    assert e_eval < TOL, e_eval
    rc, rc_ref = float(rc.cpu().reshape(-1)[0]), float(rc_ref.reshape(-1)[0])
    assert abs(rc - rc_ref) <= TOL * max(1.0, abs(rc_ref)), (rc, rc_ref)
    # one dropout-free training step
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    clf.train()
    tr = Trainer(clf, base_seed=7)
    with _lib.launch_log() as log:
        logits = tr.forward_backward(xt.cuda(), yt.cuda().reshape(-1), wt.cuda().reshape(-1), 1.0, 0.05, r_chrom)
        torch.cuda.synchronize()
    ran = {k for k, n in log.counts.items() if n > 0}
    _assert_kernels(ran, sort_must, sort_not, f"train/{size}")
    _, bce, recon, ref_logits, grads = O.loss_and_grads(P, fe, xt, yt, wt, 1.0, 0.05, random_chrom=r_chrom)
    e_logit = logit_err(logits.cpu().numpy(), ref_logits.numpy())
    assert e_logit < TOL, e_logit
    assert abs(float(tr.losses[0]) - float(bce)) <= TOL * max(1.0, abs(float(bce)))
    assert abs(float(tr.losses[1]) - float(recon[0])) <= TOL * max(1.0, abs(float(recon[0])))
    worst, worst_chunk = _check_grads(_trainer_grads(tr, clf), grads, num, r_chrom, f"c63/{size}")
    print(f"adj 63 chromosomes {size} ({xt.numel()} token slots): eval logits {e_eval:.1e}, step logits {e_logit:.1e}, worst gradient "
          f"{worst:.1e}, worst 64-chunk {worst_chunk:.1e}; kernels {sorted(k for k in ran if k.startswith('adj_'))}")


def test_adj_64_chromosomes_refused():
    """One chromosome over kMaxChrom: the library refuses the forward and the training step with its n_chrom error (a Python exception),
    before any adj kernel is launched."""
    from matcha_amd.engine import Trainer
    num = [3 + i % 5 for i in range(64)]
    N = int(np.sum(num))
    xt, yt, wt = _mixed_batch(N, 8, 64)
    clf, _ = hip_model(num, 64, "adj", 23)
    clf.eval()
    np.random.seed(5)
    with pytest.raises(_lib.MatchaHipError, match=r"n_chrom=64 outside 1\.\.63"), _lib.launch_log() as log, torch.no_grad():
        clf(xt, return_recon=True)
    torch.cuda.synchronize()
    assert not any(k.startswith("adj_") for k, n in log.counts.items() if n > 0), log.counts
    clf.train()
    tr = Trainer(clf)
    with pytest.raises(_lib.MatchaHipError, match=r"n_chrom=64 outside 1\.\.63"), _lib.launch_log() as log:
        tr.forward_backward(xt.cuda(), yt.cuda().reshape(-1), wt.cuda().reshape(-1), 1.0, 0.05, 3)
    torch.cuda.synchronize()
    assert not any(k.startswith("adj_") for k, n in log.counts.items() if n > 0), log.counts
