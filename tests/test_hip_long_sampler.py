"""The membership set and the negative sampler for rows of 9 to 32 nodes on the GPU (matcha_hashset_build_long, matcha_hashset_contains_long,
matcha_neg_sample_long; neg_sample_long_kernel: 32 lanes per negative, lane i = position i) and the loop that puts them in front of the long
training pair (matcha_amd/finetune.py): bit for bit against the plain-Python twin tests/sampler_long_ref.py, the new kernel against the old one
on identical input, exact membership at width 25, the distribution against the reference's own generate_negative
(tests/golden/sampler_stats_long.npz), the edges, and three steps of LongRowSession against the fp32 oracle.  GPU only (-m gpu)."""
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd.sampler import HyperedgeSet, NegativeSampler
from oracle import sampler as OS
from tests import sampler_long_ref as SL
from tests.test_cpu_long_sampler import long_statistics_against_reference

pytestmark = pytest.mark.gpu

TOL = 1e-4               # tests/test_hip_long_train.py::test_ten_adamw_steps_match_the_oracle: worst parameter rel_err after AdamW steps
BETA = 0.001


def _tuples(rows):
    return {tuple(int(v) for v in r if v) for r in rows}


def _rows(rng, N, ks, L):
    x = np.zeros((len(ks), L), dtype=np.int64)
    for b, k in enumerate(ks):
        x[b, :k] = np.sort(rng.choice(N, size=k, replace=False) + 1)
    return x


# ---- 1. bit for bit against the twin ------------------------------------------------------------------------------------------------------------
def mixed_case(layout, L, min_dis):
    """67 positives that mix k = 0, 1, 2, 8, 9, L - 1, L (plus 40 more known rows that are not in the batch).  A row is KNOWN -- and so redrawn
    -- when all its gaps exceed min_dis and a redraw can succeed within a few trials; every other row is a non-member and must come back as
    it is.  On "tiny" (4 chromosomes of 16 bins) a row of 31 or 32 nodes puts ~8 nodes into every chromosome: each of its ~16 redrawn nodes
    lands on another node of the row with probability ~1/2, so a duplicate-free candidate takes ~2^16 trials -- the limit -- and with
    min_dis 2 a row of more than 9 nodes has hardly any admissible candidate at all.  There the twin (plain Python, ~30 us per trial) would
    spend minutes on what the deterministic exhaustion test below pins with one row, so on "tiny" the known rows are those of k <= 17
    (min_dis 0) or k <= 9 (min_dis 2); on hg38 1 Mb every admissible row is known, k = L = 32 (the full 32-bit mask) included."""
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(1000 + 37 * L + min_dis)
    ks = [0, 1, 2, 8, 9, L - 1, L]
    batch = _rows(rng, N, [ks[i % len(ks)] for i in range(67)], L)
    extra = _rows(rng, N, [ks[1 + i % (len(ks) - 1)] for i in range(40)], L)
    k_cap = L if layout != "tiny" else (17 if min_dis == 0 else 9)
    pool = np.concatenate([batch, extra])
    kk = (pool != 0).sum(1)
    ok = np.array([k >= 1 and k <= k_cap and (k < 2 or (np.diff(r[:k]) > min_dis).all()) for r, k in zip(pool, kk)])
    known_rows = np.ascontiguousarray(pool[ok][::-1])                    # insertion order differs from the batch order
    return num, batch, known_rows, _tuples(known_rows)


@pytest.mark.parametrize("min_dis", [0, 2])
@pytest.mark.parametrize("L", [9, 17, 32])
@pytest.mark.parametrize("layout", ["tiny", "hg38_1mb"])
def test_long_sampler_bit_exact_vs_twin(layout, L, min_dis):
    num, batch, known_rows, known = mixed_case(layout, L, min_dis)
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    hs = HyperedgeSet(torch.from_numpy(known_rows).cuda())
    n_known = sum(1 for r in batch if tuple(int(v) for v in r if v) in known)
    assert 20 <= n_known < 67                                             # members and non-members
    pos = torch.from_numpy(batch).cuda()
    for neg_num, P in ((3, 67), (1, 1)):                                  # 201 negatives: not a multiple of 8, the last block is partly empty
        p = batch[2:2 + P] if P == 1 else batch                          # the single positive has k = 2
        smp = NegativeSampler(hs, n2c, cr, neg_num=neg_num, min_dis=min_dis, seed=70)
        with _lib.launch_log() as log:
            neg1 = smp.sample(torch.from_numpy(p).cuda()).cpu().numpy()
            neg2 = smp.sample(torch.from_numpy(p).cuda()).cpu().numpy()   # the next seed
        assert log.counts.get("neg_sample_long_kernel") == 2 and "neg_sample_kernel" not in log.counts, log.counts
        for seed, neg in ((71, neg1), (72, neg2)):
            ref, status = SL.sample_negatives_long(p, known, n2c, cr, neg_num, min_dis, seed, return_status=True)
            assert np.array_equal(neg, ref), (neg_num, seed, np.nonzero((neg != ref).any(1))[0][:8])
            assert status[0] == 0
            if status[1] == 0:                                            # (an exhausted negative equals its positive)
                SL.check_invariants(p, neg, known, n2c, neg_num, min_dis)
        assert not np.array_equal(neg1, neg2)
        assert smp.check_status() >= 0
    assert pos.shape == (67, L)


# ---- 2. the new kernel against the old one ------------------------------------------------------------------------------------------------------
def _sample_direct(name, hs, pos, n2c, cr, neg_num, min_dis, seed):
    """One of the two sampler entry points called directly on the same device buffers."""
    lib = _lib.load()
    dev = pos.device
    n2c_t = torch.as_tensor(np.asarray(n2c, dtype=np.int32), device=dev)
    cr_t = torch.as_tensor(np.asarray(cr, dtype=np.int32), device=dev).contiguous()
    seed_t = torch.full((1,), seed, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    neg = torch.empty(pos.shape[0] * neg_num, pos.shape[1], dtype=torch.long, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(getattr(lib, name)(_lib.ptr(hs.table), _lib.ptr(hs.edges), hs.n, hs.L, _lib.ptr(pos), pos.shape[0], pos.shape[1], neg_num, min_dis,
                                  _lib.ptr(n2c_t), n2c_t.numel() - 1, _lib.ptr(cr_t), cr_t.shape[0], _lib.ptr(seed_t), _lib.ptr(neg),
                                  _lib.ptr(status), st), name)
    return neg.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("layout,ks,min_dis", [("tiny", [2, 3], 0), ("c1", [2, 3, 4, 5], 0), ("c1", [3], 2), ("c1", [2, 5, 8], 0)])
def test_long_kernel_equals_the_short_kernel_and_the_oracle_at_up_to_8_columns(layout, ks, min_dis):
    """The rows of tests/test_hip_sampler.py::test_sampler_bit_exact_vs_oracle (L = 3, 5, 3) and one case at L = 8: with stride 8 the new kernel
    draws what neg_sample_kernel draws, so the three agree bit for bit."""
    from tests.test_hip_sampler import _setup
    num, N, L, pool = _setup(layout, ks, 150 if layout == "tiny" else 400, 3)
    known = _tuples(pool)
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    hs = HyperedgeSet(torch.from_numpy(pool).cuda())
    pos_h = pool[np.random.default_rng(2).permutation(len(pool))[:200]]
    pos = torch.from_numpy(pos_h).cuda()
    with _lib.launch_log() as log:
        new, st_new = _sample_direct("matcha_neg_sample_long", hs, pos, n2c, cr, 3, min_dis, 42)
        old, st_old = _sample_direct("matcha_neg_sample", hs, pos, n2c, cr, 3, min_dis, 42)
    assert log.counts == {"neg_sample_long_kernel": 1, "neg_sample_kernel": 1}, log.counts
    assert np.array_equal(new, old) and np.array_equal(st_new, st_old)
    assert np.array_equal(new, OS.sample_negatives(pos_h, known, n2c, cr, 3, min_dis, seed=42))


def test_one_table_format_a_width_8_set_and_a_width_32_set_give_the_same_negatives():
    num = synth.LAYOUTS["c1"]
    N = int(np.sum(num))
    rng = np.random.default_rng(5)
    pool = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, 300), ((0, 0), (0, 5 - k))) for k in (2, 3, 5)])
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    pos = torch.from_numpy(pool[rng.permutation(len(pool))[:203]]).cuda()
    out = {}
    for W in (8, 32):
        hs = HyperedgeSet(torch.from_numpy(np.pad(pool, ((0, 0), (0, W - 5)))).cuda())
        smp = NegativeSampler(hs, n2c, cr, neg_num=3, min_dis=0, seed=9)
        with _lib.launch_log() as log:
            out[W] = smp.sample(pos).cpu().numpy()
        assert set(log.counts) == ({"neg_sample_kernel"} if W == 8 else {"neg_sample_long_kernel"}), log.counts       # the routing rule
        assert smp.check_status() == 0
    assert np.array_equal(out[8], out[32])
    assert np.array_equal(out[8], OS.sample_negatives(pos.cpu().numpy(), _tuples(pool), n2c, cr, 3, 0, seed=10))
    # ... and a table BUILT by the long entry is read by the short sampler entry (width bound met: both widths <= 8 at the call)
    hs32 = HyperedgeSet(torch.from_numpy(np.pad(pool, ((0, 0), (0, 27)))).cuda())
    hs8 = HyperedgeSet(torch.from_numpy(np.pad(pool, ((0, 0), (0, 3)))).cuda())
    hs8.table = hs32.table                                                # the same rows in the same order, 8 wide; the table of the 32-wide build
    got, _ = _sample_direct("matcha_neg_sample", hs8, pos, n2c, cr, 3, 0, 10)
    assert np.array_equal(got, out[8])


# ---- 3. the set ---------------------------------------------------------------------------------------------------------------------------------
def test_membership_is_exact_at_width_25():
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    rng = np.random.default_rng(12)
    pool = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, 1500), ((0, 0), (0, 25 - k))) for k in (3, 9, 12, 25)])
    known = _tuples(pool)
    with _lib.launch_log() as log:
        hs = HyperedgeSet(torch.from_numpy(pool).cuda())
        assert bool(hs.contains(torch.from_numpy(pool)).all())                              # members
    assert log.counts == {"hashset_clear_kernel": 1, "hashset_insert_kernel": 1, "hashset_contains_kernel": 1}, log.counts
    # 20 000 queries that are members only by accident, mixed with 500 members, in one call
    q = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, 5000), ((0, 0), (0, 25 - k))) for k in (3, 9, 12, 25)] + [pool[::12]])
    q = q[rng.permutation(len(q))]
    ref = np.array([tuple(int(v) for v in r if v) in known for r in q])
    assert ref.sum() >= 500 and (~ref).sum() >= 19990
    assert np.array_equal(hs.contains(torch.from_numpy(q)).cpu().numpy(), ref)
    # a k = 9 prefix of a k = 12 member is another hyperedge
    pre = pool[(pool != 0).sum(1) == 12][:200].copy()
    pre[:, 9:] = 0
    refp = np.array([tuple(int(v) for v in r if v) in known for r in pre])
    assert not refp.any()
    assert np.array_equal(hs.contains(torch.from_numpy(pre)).cpu().numpy(), refp)
    assert np.array_equal(hs.contains(torch.from_numpy(pre[:, :9].copy())).cpu().numpy(), refp)
    # duplicates in the input are fine
    hs2 = HyperedgeSet(torch.from_numpy(np.concatenate([pool[-50:], pool[-50:], pool[:50]])).cuda())
    assert bool(hs2.contains(torch.from_numpy(pool[-50:])).all()) and bool(hs2.contains(torch.from_numpy(pool[:50])).all())
    assert not bool(hs2.contains(torch.from_numpy(pool[50:100])).any())


def test_narrow_queries_on_a_wide_set_and_wide_queries_on_a_narrow_set():
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    rng = np.random.default_rng(13)
    small = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, 400), ((0, 0), (0, 5 - k))) for k in (2, 3, 5)])
    big = np.pad(synth.make_edges_fast(rng, N, 12, 400), ((0, 0), (0, 13)))
    wide = HyperedgeSet(torch.from_numpy(np.concatenate([np.pad(small[::2], ((0, 0), (0, 20))), big])).cuda())       # width 25
    narrow = HyperedgeSet(torch.from_numpy(small[::2].copy()).cuda())                                                    # width 5
    ref = np.arange(len(small)) % 2 == 0
    # a stored row of k <= 5 nodes in the width-25 set is found by a width-5 query (and a width-8 one)
    assert np.array_equal(wide.contains(torch.from_numpy(small)).cpu().numpy(), ref)
    assert np.array_equal(wide.contains(torch.from_numpy(np.pad(small, ((0, 0), (0, 3))))).cpu().numpy(), ref)
    # width-25 and width-32 queries on the width-5 set: the short rows are found, a row of 12 nodes never is
    with _lib.launch_log() as log:
        assert np.array_equal(narrow.contains(torch.from_numpy(np.pad(small, ((0, 0), (0, 20))))).cpu().numpy(), ref)
        assert np.array_equal(narrow.contains(torch.from_numpy(np.pad(small, ((0, 0), (0, 27))))).cpu().numpy(), ref)
        assert not bool(narrow.contains(torch.from_numpy(big)).any())
        five = big.copy()
        five[:, 5:] = 0                                                                     # the 5-prefix of a 12-row, 25 wide: not stored either
        assert not bool(narrow.contains(torch.from_numpy(five)).any())
    assert log.counts == {"hashset_contains_kernel": 4}, log.counts
    # a build and a query at L <= 8 log the kernels they always did
    with _lib.launch_log() as log:
        hs = HyperedgeSet(torch.from_numpy(small).cuda())
        assert bool(hs.contains(torch.from_numpy(small)).all())
        HyperedgeSet.empty("cuda", 5)
    assert log.counts == {"hashset_clear_kernel": 2, "hashset_insert_kernel": 1, "hashset_contains_kernel": 1}, log.counts


# ---- 4. statistics against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_dis", [0, 2])
def test_long_sampler_distribution_vs_reference_and_invariants(min_dis):
    """The batch of tests/golden/sampler_stats_long.npz (hg38 1 Mb, k in {9, 12, 16, 25} padded to 25, 4 000 positives, neg_num 3): every
    invariant of generate_negative on all 12 000 negatives, and per k the differing-node and replaced-position histograms against the
    reference's own, two-sample chi-square below chi2.isf(1e-6, bins - 1) (tests/test_cpu_long_sampler.py states the test and the twin's
    figures; the kernel draws the twin's stream, at another seed).

    Measured on the MI355X (seed 21) -- chi2 [bins used; bound] of the differing-node / replaced-position histograms:
      min_dis 0: k 9  12.35 [9; 42.70] / 1.43 [9; 42.70]     k 12 15.09 [12; 48.87] / 3.90 [12; 48.87]
                 k 16 12.93 [13; 50.83] / 14.85 [16; 56.49]  k 25 15.95 [15; 54.64] / 10.93 [25; 72.23]
      min_dis 2: k 9  8.01 [9; 42.70] / 2.61 [9; 42.70]      k 12 10.71 [11; 46.86] / 0.98 [12; 48.87]
                 k 16 15.21 [13; 50.83] / 5.57 [16; 56.49]   k 25 20.99 [17; 58.32] / 11.53 [25; 72.23]"""
    num = synth.LAYOUTS["hg38_1mb"]
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    batch, known, known_rows = SL.long_sampler_case(min_dis)
    hs = HyperedgeSet(torch.from_numpy(known_rows).cuda())
    smp = NegativeSampler(hs, n2c, cr, neg_num=3, min_dis=min_dis, seed=20)
    neg = smp.sample(torch.from_numpy(batch).cuda()).cpu().numpy()
    assert smp.check_status() == 0
    assert SL.check_invariants(batch, neg, known, n2c, 3, min_dis) == len(neg) == 12000
    long_statistics_against_reference(batch, neg, min_dis)


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_set_copies_the_positives():
    num = synth.LAYOUTS["c1"]
    pos = _rows(np.random.default_rng(0), int(np.sum(num)), [12, 9, 25, 2, 0, 1] * 11, 25)
    smp = NegativeSampler(HyperedgeSet.empty("cuda", 25), synth.node2chrom(num), synth.chrom_range(num), neg_num=3, seed=1)
    with _lib.launch_log() as log:
        neg = smp.sample(torch.from_numpy(pos).cuda()).cpu().numpy()
    assert log.counts == {"neg_sample_long_kernel": 1}
    assert np.array_equal(neg, np.repeat(pos, 3, axis=0)) and smp.check_status() == 0


def test_a_node_without_a_chromosome_is_a_key_error():
    num = synth.LAYOUTS["c1"]
    N = int(np.sum(num))
    pos = _rows(np.random.default_rng(1), N, [9, 12, 10], 12)
    n2c = synth.node2chrom(num).copy()
    n2c[pos[1, :12]] = -1                                                 # the whole second row: whichever positions its masks choose
    smp = NegativeSampler(HyperedgeSet(torch.from_numpy(pos).cuda()), n2c, synth.chrom_range(num), neg_num=3, seed=1)
    neg = smp.sample(torch.from_numpy(pos).cuda()).cpu().numpy()
    with pytest.raises(KeyError, match="without a chromosome"):
        smp.check_status()
    assert smp.check_status() == 0                                        # the word was cleared
    assert (np.diff(neg[[0, 1, 2, 6, 7, 8], :9]) > 0).all()               # the other rows were redrawn all the same


def test_exhausted_trials_return_the_positive_and_are_counted():
    """Deterministic: on "tiny" the 16 nodes of chromosome 0 as one known row.  Whatever is redrawn stays in 1..16, so a duplicate-free
    candidate is the positive itself, which is known: all 65 536 trials are rejected, the row comes back equal to its positive and
    status[1] counts it -- once, not once per lane.  The row beside it (k = 3) is redrawn as usual."""
    num = synth.LAYOUTS["tiny"]
    pos = np.zeros((2, 17), dtype=np.int64)
    pos[0, :16] = np.arange(1, 17)
    pos[1, :3] = [20, 40, 60]
    smp = NegativeSampler(HyperedgeSet(torch.from_numpy(pos).cuda()), synth.node2chrom(num), synth.chrom_range(num), neg_num=1, seed=3)
    neg = smp.sample(torch.from_numpy(pos).cuda()).cpu().numpy()
    assert np.array_equal(neg[0], pos[0])
    assert not np.array_equal(neg[1], pos[1]) and (np.diff(neg[1, :3]) > 0).all() and (neg[1, 3:] == 0).all()
    assert smp.check_status() == 1


def test_width_33_is_a_value_error_before_any_launch():
    num = synth.LAYOUTS["c1"]
    hs = HyperedgeSet.empty("cuda", 32)
    smp = NegativeSampler(hs, synth.node2chrom(num), synth.chrom_range(num))
    with _lib.launch_log() as log:
        with pytest.raises(ValueError, match="33 columns"):
            HyperedgeSet(torch.ones((4, 33), dtype=torch.long, device="cuda"))
        with pytest.raises(ValueError, match="33 columns"):
            HyperedgeSet.empty("cuda", 33)
        with pytest.raises(ValueError, match="33 columns"):
            hs.contains(torch.ones((4, 33), dtype=torch.long))
        with pytest.raises(ValueError, match="33 columns"):
            smp.sample(torch.ones((4, 33), dtype=torch.long, device="cuda"))
        with pytest.raises(ValueError, match="33 columns"):
            smp.sample_into(torch.ones((4, 33), dtype=torch.long, device="cuda"), torch.empty((12, 33), dtype=torch.long, device="cuda"))
    assert not log.counts, log.counts


# ---- 6. the loop --------------------------------------------------------------------------------------------------------------------------------
def _tiny_model(mode):
    from tests.helpers import oracle_state
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["tiny"]
    _, fe, sd = oracle_state(num, 16, mode, 77)
    clf, _ = hip_model(num, 16, mode, 77, sd=sd)
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return num, clf, fe, sd


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_three_steps_of_the_long_row_session_match_the_oracle(mode):
    """LongRowSession.step at L = 12, P = 12, neg_num 3 (48 rows): the batches the session recorded go through the fp32 oracle under the same
    torch.optim.AdamW with the same chromosome draws; parameters after steps 1 and 3 within the bound of
    tests/test_hip_long_train.py::test_ten_adamw_steps_match_the_oracle (worst rel_err <= 1e-4, the gauge direction left out)."""
    from matcha_amd.finetune import LongRowSession
    from oracle import hypersagnn as O
    from tests import fp64_grade as G
    from tests.helpers import rel_err
    num, clf, fe, sd = _tiny_model(mode)
    N = int(np.sum(num))
    rng = np.random.default_rng(612)
    known = _rows(rng, N, [12, 2, 9, 5, 10, 3, 12, 8, 4, 11, 7, 6] * 3, 12)
    sess = LongRowSession(clf, known, synth.node2chrom(num), synth.chrom_range(num), neg_num=3, min_dis=0, lr=1e-3, seed=5)
    assert clf.long_row_training is True
    P = {k: torch.from_numpy(np.array(v)).requires_grad_(k not in G.FROZEN_NAMES) for k, v in sd.items()}
    names = [n for n, t in P.items() if t.requires_grad]
    opt_o = torch.optim.AdamW([P[n] for n in names], lr=1e-3)
    np.random.seed(77)
    chroms = [int(np.random.choice(np.arange(len(num)), 1)[0]) for _ in range(3)]
    np.random.seed(77)
    for it in range(3):
        pos = torch.from_numpy(known[12 * it:12 * it + 12]).cuda()
        pw = torch.from_numpy((0.5 + 1.5 * rng.random(12)).astype(np.float32)).cuda()
        with _lib.launch_log() as log:
            bce, recon, logits, y, sizes = sess.step(pos, pw, alpha=1.0, beta=BETA)
        assert {"neg_sample_long_kernel", "attn_long_kernel", "attn_long_bwd_kernel"} <= set(log.counts), log.counts
        x, yb, wb, sb = sess.last_batch
        # generate_negative's layout (main.py:443-448)
        assert x.shape == (48, 12) and torch.equal(x[:12], pos) and logits.shape == (48,) and bce.dim() == 0 and bce.is_cuda
        assert torch.equal(yb, torch.cat([torch.ones(12), torch.zeros(36)]).cuda()) and yb is y
        assert torch.equal(wb, torch.cat([pw, torch.ones(36, device="cuda")]))
        assert torch.equal(sb, (x != 0).sum(1)) and torch.equal(sb[12:], sb[:12].repeat_interleave(3)) and sb is sizes
        assert not torch.equal(x[12:], pos.repeat_interleave(3, dim=0))                      # known positives: redrawn
        xh, yh, wh = x.cpu(), yb.cpu().view(-1, 1), wb.cpu().view(-1, 1)
        lg, rc = O.classifier_forward(P, fe, xh, random_chrom=chroms[it])
        opt_o.zero_grad()
        loss_o = O.bce_with_logits(lg, yh, wh)
        (loss_o + rc * BETA).backward()
        opt_o.step()
        assert abs(float(bce) - float(loss_o.detach())) <= TOL * max(1.0, abs(float(loss_o.detach())))
        if it in (0, 2):
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
    assert sess.check_status() == 0


def test_the_session_at_width_5_takes_the_short_path():
    from matcha_amd.finetune import LongRowSession
    num, clf, fe, sd = _tiny_model("table")
    N = int(np.sum(num))
    rng = np.random.default_rng(613)
    known = _rows(rng, N, [5, 2, 3, 4] * 6, 5)
    sess = LongRowSession(clf, known, synth.node2chrom(num), synth.chrom_range(num), neg_num=3, seed=5)
    before = {n: p.detach().clone() for n, p in clf.named_parameters()}
    with _lib.launch_log() as log:
        bce, recon, logits, y, sizes = sess.step(torch.from_numpy(known[:12]).cuda(), torch.ones(12, device="cuda"))
        ev = sess.eval_epoch(known, np.ones(len(known), dtype=np.float32), batch_size=12)
    assert "neg_sample_kernel" in log.counts and not [k for k in log.counts if "long" in k], log.counts
    assert logits.shape == (48,) and np.isfinite(float(bce))
    assert any(not torch.equal(before[n], p.detach()) for n, p in clf.named_parameters())   # AdamW stepped
    assert len(ev) == 5 and np.isfinite(ev[0]) and clf.training                              # eval_epoch restores the mode


def test_finetune_command_line_writes_the_checkpoint_and_the_model(tmp_path):
    """python -m matcha_amd.finetune in process: all_<k>_counter.npy for k = 9 and 12 on "tiny", a pickled model2load, one epoch of
    24-positive batches -> OUT/model.chkpt and OUT/model2load that load back with moved parameters."""
    import os
    from matcha_amd import finetune as FT
    from tests.test_train_driver import _write_temp_dir
    cfg, num = _write_temp_dir(str(tmp_path), layout="tiny", ks=(9, 12), m=150)
    _, clf, fe, sd = _tiny_model("table")
    path = os.path.join(cfg["temp_dir"], "model2load")
    torch.save(clf, path)
    out = os.path.join(str(tmp_path), "OUT")
    np.random.seed(3)
    with _lib.launch_log() as log:
        FT.main(["--config", os.path.join(str(tmp_path), "config.JSON"), "--model", path, "--sizes", "9", "12", "--epochs", "1",
                 "--batch-size", "24", "-o", out])
    assert {"neg_sample_long_kernel", "attn_long_bwd_kernel", "attn_long_kernel"} <= set(log.counts), log.counts
    ck = torch.load(os.path.join(out, "model.chkpt"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 0
    tuned = torch.load(os.path.join(out, "model2load"), map_location="cuda", weights_only=False)
    name = "encode1.mul_head_attn.w_qs.weight"
    assert not np.array_equal(ck["model_link"][name].numpy(), np.array(sd[name]))             # AdamW stepped
    assert torch.equal(dict(tuned.named_parameters())[name].detach().cpu(), ck["model_link"][name])
    with torch.no_grad():
        tuned.eval()
        assert torch.isfinite(tuned(torch.from_numpy(_rows(np.random.default_rng(1), 64, [12, 9, 3], 12)).cuda())).all()
