"""The anchored k-way sweep on the MI355X (csrc/sweep_rows.hip, csrc/sweep_select.hip, matcha_amd/sweep.py): anchored candidate rows and their
flags bit for bit against itertools and, beyond 2^40, against anchored_unrank; the segmented selection bit for bit against numpy's
lexsort however the stream is cut; the sweep against the reference's own logits per anchor (g11) and against one batch per anchor
of the d = 64 model with partners on another chromosome; the CLI."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd import predict as PR
from matcha_amd import sweep as SW
from matcha_amd.sampler import HyperedgeSet
from tests import denoise_ref as R
from tests.helpers import GOLD, gold
from tests.test_cpu_kanchor import CLOSE_PAIR, GRID, PAIR_OFFSETS, anchor_cases, anchor_ksel, brute_anchored
from tests.test_hip_kway import TOL, d64, load_tiny, run_topk, salted_scores, same_bits  # noqa: F401  (d64 is a fixture)

pytestmark = pytest.mark.gpu

SEG_KERNELS = {"segtopk_keys_kernel", "segtopk_merge_kernel", "segtopk_commit_kernel"}


def table_ref(anchors, lo, n, k, g, width=None):
    """(rows int64 [A * C_f, width], invalid bool [A * C_f]) of an anchor table in global-rank order, by brute force."""
    rows, bad = [], []
    for anchor in anchors:
        for row, ok in brute_anchored(list(anchor), lo, n, k, g):
            rows.append(row)
            bad.append(not ok)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, k)
    return np.pad(rows, ((0, 0), (0, (width or k) - k))), np.asarray(bad, dtype=bool)


def got_np(pair):
    x, flag = pair
    assert x.dtype == torch.long and flag.dtype == torch.int32 and flag.shape == (x.shape[0],)
    return x.cpu().numpy(), flag.cpu().numpy() != 0


# ---- rows, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_rows_grid(wide):
    for lo, n, k, s, g in GRID:
        anchors = list(anchor_cases(lo, n, s, g).values())
        width = 8 if wide else k
        ref, bad = table_ref(anchors, lo, n, k, g, width)
        with _lib.launch_log() as log:
            x, inv = got_np(SW.anchored_rows(np.asarray(anchors), lo, n, k, g, width=width))
        assert x.shape == ref.shape and np.array_equal(x, ref) and np.array_equal(inv, bad), (lo, n, k, s, g)
        if len(ref) == 0:                                                # a region too small for the free part: nothing to launch
            assert not log.counts
            continue
        assert set(log.counts) == {"kway_anchor_rows_kernel"}            # it, and only it
        assert bad.any() and not bad.all()


@pytest.mark.parametrize("k,s,g", [(2, 1, 1), (3, 1, 2), (4, 2, 3), (4, 1, 1)])
def test_rows_ranges_inside_and_across_segments(k, s, g):
    """40 anchors inside and outside the region [5, 21): ranges that start and end inside a segment (one anchor's C_f ranks) and that
    cross one or many segment boundaries; counts around a wave and over the 256-row block."""
    lo, n = 5, 16
    anchors = np.asarray([[a + 5 * j for j in range(s)] for a in range(1, 41)], dtype=np.int64)
    ref, bad = table_ref(anchors, lo, n, k, g, 6)
    cf = len(ref) // 40
    assert cf == SW.anchored_count(1, s, n, k, g) and len(ref) == SW.anchored_count(40, s, n, k, g)
    dev_anchors = torch.from_numpy(anchors).cuda()
    crossed = set()
    ranges = [(2 * cf - 2, 5)]                                           # over exactly one boundary whatever C_f (>= 16 here)
    for count in (1, 63, 64, 65, 300, 513):
        for base in (1, 3 * cf + cf // 3, len(ref) - count - cf):
            ranges.append((next(r for r in range(base, base + cf) if r % cf and (r + count) % cf), count))
    for rank0, count in ranges:
        assert rank0 % cf and (rank0 + count) % cf                       # begins and ends inside a segment
        x, inv = got_np(SW.anchored_rows(dev_anchors, lo, n, k, g, rank0=rank0, count=count, width=6))
        assert np.array_equal(x, ref[rank0:rank0 + count]) and np.array_equal(inv, bad[rank0:rank0 + count]), (rank0, count)
        crossed.add(min((rank0 + count - 1) // cf - rank0 // cf, 2))
    assert {0, 1} <= crossed and (cf > 200 or 2 in crossed)              # inside one segment, over one boundary, over several
    with pytest.raises(IndexError):
        SW.anchored_rows(dev_anchors, lo, n, k, g, rank0=len(ref) - 1, count=2)


def test_rows_list_form_and_reused_buffers():
    lo, n, k, s, g = 5, 16, 4, 2, 2
    anchors = np.asarray(list(anchor_cases(lo, n, s, g).values()), dtype=np.int64)
    ref, bad = table_ref(anchors, lo, n, k, g, 6)
    total = len(ref)
    rng = np.random.default_rng(5)
    ranks = np.concatenate([rng.permutation(total), rng.integers(0, total, 300), [-1, total, 1 << 62, -(1 << 40), 0, total - 1]])
    rng.shuffle(ranks)
    with _lib.launch_log() as log:
        x, inv = got_np(SW.anchored_rows(anchors, lo, n, k, g, ranks=torch.from_numpy(ranks).cuda(), width=6))
    assert log.counts == {"kway_anchor_rows_kernel": 1}                  # the same kernel as the range form
    ok = (ranks >= 0) & (ranks < total)
    assert np.array_equal(x[ok], ref[ranks[ok]]) and np.array_equal(inv[ok], bad[ranks[ok]])
    assert not x[~ok].any() and inv[~ok].all() and (~ok).sum() == 4      # out of range: a zero row with its flag set
    # no anchors, or a region without candidates: every listed rank is out of range
    for table, region in ((np.zeros((0, 2), dtype=np.int64), (lo, n)), (anchors, (1, 2))):
        x, inv = got_np(SW.anchored_rows(table, *region, k, g, ranks=torch.tensor([0, 1], device="cuda")))
        assert not x.any() and inv.all()
        assert SW.anchored_rows(table, *region, k, g, device="cuda")[0].shape == (0, k)
    # ``out`` and ``flag_out`` reuse the caller's buffers and leave their tails alone
    buf = torch.full((100 * 6,), -7, dtype=torch.long, device="cuda")
    fbuf = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    x, flag = SW.anchored_rows(anchors, lo, n, k, g, rank0=10, count=40, width=6, out=buf, flag_out=fbuf)
    assert x.data_ptr() == buf.data_ptr() and flag.data_ptr() == fbuf.data_ptr()
    assert np.array_equal(x.cpu().numpy(), ref[10:50]) and np.array_equal(flag.cpu().numpy() != 0, bad[10:50])
    assert bool((buf[240:] == -7).all()) and bool((fbuf[40:] == -7).all())


def test_rows_large_ranks_against_unrank():
    lo, n, k, g = 3000, 2491, 5, 2
    cf = SW.anchored_count(1, 1, n, k, g)
    assert cf > 1 << 40
    A = (1 << 62) // cf
    total = SW.anchored_count(A, 1, n, k, g)
    assert (1 << 62) - cf < total <= 1 << 62
    ids = (np.arange(A, dtype=np.int64) * 7) % 6000 + 1                  # below, inside and above the region
    anchors = torch.from_numpy(ids).cuda().view(-1, 1)
    ranks = [0, cf - 1, cf, (1 << 40) + 12345, total // 3, total // 2 + 1, total - cf, total - 1]
    x, inv = got_np(SW.anchored_rows(anchors, lo, n, k, g, ranks=torch.tensor(ranks, device="cuda")))
    for r, row, bad in zip(ranks, x, inv):
        want, ok = SW.anchored_unrank(r % cf, [int(ids[r // cf])], lo, n, k, g)
        assert tuple(row) == want and bool(bad) == (not ok), r
    # a run of 1000 inside one segment: every row holds the anchor, is sorted, its flag is the gap rule, and the free parts follow
    # each other as lexicographic successors
    for a, r in ((A - 1, cf - 1000), (A // 2, cf // 7)):
        anchor = int(ids[a])
        x, inv = got_np(SW.anchored_rows(anchors, lo, n, k, g, rank0=a * cf + r, count=1000))
        assert (np.diff(x, axis=1) >= 0).all() and np.array_equal(inv, (np.diff(x, axis=1) < g).any(axis=1))
        free = []
        for row in x.tolist():
            row.remove(anchor)
            free.append(row)
        y = np.asarray(free) - lo - np.arange(k - 1) * (g - 1)
        m = n - (k - 2) * (g - 1)
        assert (np.diff(y, axis=1) > 0).all() and y.min() >= 0 and y.max() < m
        for p, q in zip(y[:-1], y[1:]):
            j = max(i for i in range(k - 1) if p[i] < m - (k - 1) + i)  # the last position that can still move
            assert np.array_equal(q[:j], p[:j]) and q[j] == p[j] + 1 and np.array_equal(q[j:], q[j] + np.arange(k - 1 - j))
        assert tuple(x[0]) == SW.anchored_unrank(r, [anchor], lo, n, k, g)[0] and tuple(x[-1]) == SW.anchored_unrank(r + 999, [anchor], lo, n, k, g)[0]
    with pytest.raises(IndexError):
        SW.anchored_rows(anchors, lo, n, k, g, rank0=total - 1, count=2)


# ---- segmented selection, exact, no model ------------------------------------------------------------------------------------------
def seg_ref(s, skip, K, seg_len, g0, first_segment, A):
    """Per segment the best K valid rows by numpy's lexsort (higher score first, -0.0 == +0.0, then lower rank), flattened segment
    by segment: (scores, global ranks, counts [A])."""
    g = g0 + np.arange(len(s), dtype=np.int64)
    seg = g // seg_len - first_segment
    valid = np.flatnonzero(~np.isnan(s) & (skip == 0))
    order = valid[np.lexsort((valid, -s[valid], seg[valid]))]
    sseg = seg[order]
    starts = np.flatnonzero(np.r_[True, sseg[1:] != sseg[:-1]]) if len(order) else np.zeros(0, dtype=np.int64)
    pos = np.arange(len(order)) - np.repeat(starts, np.diff(np.r_[starts, len(order)]))
    order, sseg = order[pos < K], sseg[pos < K]
    return s[order], g[order], np.bincount(sseg, minlength=A).astype(np.int64)


def check_seg(sel, ref):
    ref_s, ref_r, ref_c = ref
    sc, rk, cnt = sel.read()
    assert sc.shape == rk.shape == (sel.A, sel.K) and cnt.shape == (sel.A,)
    assert np.array_equal(cnt.cpu().numpy(), ref_c)
    kept = torch.arange(sel.K, device=cnt.device).view(1, -1) < cnt.view(-1, 1)
    assert np.array_equal(rk[kept].cpu().numpy(), ref_r)
    assert same_bits(sc[kept].cpu().numpy(), ref_s)                      # the kept score keeps its bits (-0.0 stays -0.0)
    assert bool((rk.masked_fill(kept, -1) == -1).all()) and bool((sc.view(torch.int32).masked_fill(kept, 0) == 0).all())


def run_seg(st, kt, A, K, seg_len, piece, g0, first_segment):
    sel = SW.SegTopK(A, K, seg_len, piece, "cuda", first_segment=first_segment)
    for a in range(0, st.numel(), piece):
        sel.update(st[a:a + piece], g0 + a, kt[a:a + piece])
    return sel


@pytest.mark.parametrize("K", [1, 7, 64, 1000])
def test_segmented_selection_exact_however_the_stream_is_cut(K):
    s, skip = salted_scores()
    n = len(s)
    for seg_len in (1, 7, 64, 1000, 100000):
        first_segment = (1 << 40) // seg_len + 1
        off = seg_len // 3                                               # the stream begins inside a segment (seg_len > 2)
        g0 = first_segment * seg_len + off
        assert g0 > 1 << 40
        touched = (off + n - 1) // seg_len + 1
        A = touched + 2                                                  # two segments the stream never reaches
        sk = skip.copy()
        if touched > 5:
            sk[max(0, 5 * seg_len - off):6 * seg_len - off] = 3          # one segment entirely skipped
        st, kt = torch.from_numpy(s).cuda(), torch.from_numpy(sk).cuda()
        ref = seg_ref(s, sk, K, seg_len, g0, first_segment, A)
        assert ref[2][touched:].sum() == 0 and (touched <= 5 or ref[2][5] == 0) and ref[2].max() <= K
        if seg_len < K:
            assert (ref[2] < K).all() and ref[2].any()                   # every segment has fewer valid rows than K
        for piece in (37, 64, 4099, n):
            check_seg(run_seg(st, kt, A, K, seg_len, piece, g0, first_segment), ref)
        # single-row updates, on the first 300 rows
        ref = seg_ref(s[:300], sk[:300], K, seg_len, g0, first_segment, A)
        for piece in (1, 300):
            check_seg(run_seg(st[:300], kt[:300], A, K, seg_len, piece, g0, first_segment), ref)


@pytest.mark.parametrize("K", [1, 64, 1000])
def test_one_segment_equals_topk(K):
    s, skip = salted_scores()
    g0 = (1 << 40) + 3
    st, kt = torch.from_numpy(s).cuda(), torch.from_numpy(skip).cuda()
    for piece in (4099, len(s)):
        ref_s, ref_r = run_topk(s, skip, K, piece, g0)
        sc, rk, cnt = run_seg(st, kt, 1, K, 1 << 41, piece, g0, 0).read()
        kept = int(cnt[0])
        assert kept == len(ref_r) and np.array_equal(rk[0, :kept].cpu().numpy(), ref_r) and same_bits(sc[0, :kept].cpu().numpy(), ref_s)


def test_segmented_selection_launches_and_empty_updates():
    rng = np.random.default_rng(2)
    s = rng.standard_normal(50).astype(np.float32)
    s[rng.choice(50, 5, replace=False)] = np.nan
    none = np.zeros(50, dtype=np.int32)
    sel = SW.SegTopK(6, 64, 10, 50, "cuda")
    sc, rk, cnt = sel.read()
    assert not cnt.any() and bool((rk == -1).all()) and not sc.any()     # nothing seen yet
    with _lib.launch_log() as log:
        sel.update(torch.zeros(0, device="cuda"), 0)                     # an empty update launches nothing
    assert not log.counts
    with _lib.launch_log() as log:
        sel.update(torch.from_numpy(s).cuda(), 5)                        # ranks 5 .. 54: segments 0 .. 5, the first and last in part
        sel.update(torch.zeros(0, device="cuda"), 55)
        sel.read()
    assert set(log.counts) == SEG_KERNELS | {"segtopk_read_kernel"} and all(v == 1 for v in log.counts.values())
    check_seg(sel, seg_ref(s, none, 64, 10, 5, 0, 6))
    with pytest.raises(_lib.MatchaHipError):
        sel.update(torch.zeros(51, device="cuda"), 0)                    # more rows than max_chunk
    with pytest.raises(_lib.MatchaHipError):
        sel.update(torch.zeros(10, device="cuda"), 55)                   # beyond the last segment
    for bad in ((6, 0, 10, 50), (0, 4, 10, 50), (6, 4, 0, 50), (6, 4, 10, 0), (1 << 16, 1 << 15, 10, 50)):
        with pytest.raises(ValueError):
            SW.SegTopK(*bad, "cuda")


def test_two_segmented_selections_alive_at_once():
    s, skip = salted_scores(5000, seed=3)
    t = np.random.default_rng(4).standard_normal(5000).astype(np.float32)
    none = np.zeros(5000, dtype=np.int32)
    a, b = SW.SegTopK(8, 100, 700, 512, "cuda"), SW.SegTopK(5000 // 3 + 1, 2, 3, 700, "cuda")
    st, kt, tt = torch.from_numpy(s).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(t).cuda()
    pa = pb = 0
    while pa < 5000 or pb < 5000:                                        # interleaved updates of different sizes
        if pa < 5000:
            a.update(st[pa:pa + 512], pa, kt[pa:pa + 512])
            pa += 512
        if pb < 5000:
            b.update(tt[pb:pb + 700], pb)
            pb += 700
    check_seg(a, seg_ref(s, skip, 100, 700, 0, 0, 8))
    check_seg(b, seg_ref(t, none, 2, 3, 0, 0, 5000 // 3 + 1))


# ---- against the reference ---------------------------------------------------------------------------------------------------------
def check_anchor_against_fixture(out, a, ids, rows, ref, scale, top):
    """One anchor of a sweep result against the fixture rows that contain ``ids`` and the reference's logits of them."""
    member = np.flatnonzero(np.all([(rows == v).any(axis=1) for v in ids], axis=0))
    index = {tuple(r): i for i, r in zip(member.tolist(), rows[member].tolist())}
    count = int(out["count"][a])
    assert count == min(top, len(member)), (ids, count, len(member))
    kept = out["rows"][a, :count].cpu().numpy()
    logit = out["logit"][a, :count].cpu().numpy()
    where = np.asarray([index[tuple(r)] for r in kept.tolist()], dtype=np.int64)       # every kept row is a fixture row (KeyError otherwise)
    assert len(set(where.tolist())) == count
    if count:
        assert float(np.abs(logit.astype(np.float64) - ref[where]).max()) / scale < TOL, ids
        assert (logit[:-1] >= logit[1:]).all()
    assert bool((out["rank"][a, count:] == -1).all()) and not out["rows"][a, count:].any() and not out["logit"][a, count:].any()
    assert not out["proba"][a, count:].any()
    if len(member) >= 3:
        K_a, _ = anchor_ksel(ref[member])
        want = set(member[np.argsort(-ref[member])[:K_a]].tolist())
        assert set(where[:K_a].tolist()) == want, ids                    # the first K_a kept rows as a set: the reference's top K_a
    return where


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_anchored_sweep_against_reference_logits(mode):
    g = gold("g11_kway_tiny.npz")
    clf = load_tiny(mode)
    cr = np.asarray(synth.chrom_range([int(v) for v in g["num"]]))
    top = 16
    for i, (c, k, gap) in enumerate(g["cases"]):
        c, k, gap = int(c), int(k), int(gap)
        lo, hi = int(cr[c][0]), int(cr[c][1])
        n = hi - lo
        rows, ref = g[f"rows_c{i}"], g[f"logit_{mode}_c{i}"].astype(np.float64)
        scale = float(np.abs(ref).max())                                 # rel_err's scale: the case's largest logit
        tables = [np.arange(lo, hi, dtype=np.int64).reshape(-1, 1)]
        if k >= 4:
            tables.append(np.asarray([(lo + a, lo + b) for a, b in PAIR_OFFSETS + [CLOSE_PAIR]], dtype=np.int64))
        for anchors in tables:
            A, s = anchors.shape
            _, bad = table_ref(anchors, lo, n, k, gap)
            first = None
            for chunk_rows in (37, 10000):
                with _lib.launch_log() as log:
                    out = SW.anchored_sweep(clf, anchors, lo, hi, k, gap, top=top, chunk_rows=chunk_rows)
                chunks = -(-len(bad) // chunk_rows)
                assert log.counts["kway_anchor_rows_kernel"] == chunks + 1 and log.counts["segtopk_merge_kernel"] == chunks
                assert {"segtopk_init_kernel", "segtopk_read_kernel"} | SEG_KERNELS <= set(log.counts) and "kway_rows_kernel" not in log.counts
                assert out["n_candidates"] == A * SW.anchored_count(1, s, n, k, gap) == len(bad)
                assert out["n_invalid"] == int(bad.sum()) and out["n_excluded"] == 0
                assert out["rows"].shape == (A, top, k) and out["logit"].shape == out["proba"].shape == out["rank"].shape == (A, top)
                for a in range(A):
                    where = check_anchor_against_fixture(out, a, anchors[a].tolist(), rows, ref, scale, top)
                    count = len(where)
                    for r, row in zip(out["rank"][a, :count].tolist(), out["rows"][a, :count].tolist()):
                        assert SW.anchored_unrank(r, anchors[a].tolist(), lo, n, k, gap) == (tuple(row), True)
                if s == 2:
                    assert int(out["count"][-1]) == 0                    # the pair closer than the gap: no valid candidate
                kept = out["rank"] >= 0
                assert torch.equal(out["proba"][kept], torch.sigmoid(out["logit"][kept]))
                if first is None:
                    first = out
                else:                                                    # the chunking is not part of the result
                    assert all(torch.equal(out[key], first[key]) for key in ("rows", "logit", "proba", "rank", "count"))


# ---- partners on another chromosome, d = 64 ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trans(d64):
    """Five single anchors on the first chromosome of hg38 at 1 Mb, the 48-bin chromosome as partner region, k = 3, min_gap = 3:
    per anchor all 1 035 candidates and ``full`` = model(all of them) in one batch, at widths 3 and 5.  A batch of 1 035 rows would
    go to the library's small-batch forward, which rounds a few ulp differently from the large-batch route the sweep pins (DESIGN.md
    7.3: up to 1.9e-6); ``full`` is computed on the pinned route too, so the 1e-6 below is again two batchings of one forward."""
    lo, hi, clf = d64["lo"], d64["hi"], d64["clf"]
    n = hi - lo
    cr = np.asarray(synth.chrom_range(synth.LAYOUTS["hg38_1mb"]))
    a_lo, a_hi = int(cr[0][0]), int(cr[0][1])
    assert a_hi + 3 <= lo                                                # another chromosome, clear of the region: every candidate valid
    anchors = np.asarray([a_lo, a_lo + 17, a_lo + 100, a_lo + 101, a_hi - 1], dtype=np.int64)
    cf = SW.anchored_count(1, 1, n, 3, 3)
    assert cf == 1035
    rows = [np.asarray([SW.anchored_unrank(r, [int(a)], lo, n, 3, 3)[0] for r in range(cf)], dtype=np.int64) for a in anchors]
    full = {3: [], 5: []}
    with torch.no_grad(), _lib.option("disable_small_batch"):
        for width in (3, 5):
            for per_anchor in rows:
                x = torch.from_numpy(np.pad(per_anchor, ((0, 0), (0, width - 3)))).cuda()
                full[width].append(clf(x).reshape(-1).clone())
    return dict(anchors=anchors, rows=rows, full=full, cf=cf, n=n)


def check_trans_top(out, trans, width, top, eligible=None):
    """check_top's properties (tests/test_hip_kway.py), per anchor."""
    assert out["rows"].shape == (5, top, width) and bool((out["count"] == top).all())
    for a in range(5):
        full, rows = trans["full"][width][a], trans["rows"][a]
        rank, logit = out["rank"][a], out["logit"][a]
        assert len(set(rank.tolist())) == top and int(rank.min()) >= 0
        assert float((logit - full[rank]).abs().max()) <= 1e-6           # what two batchings of one forward may differ by
        assert bool((logit[:-1] >= logit[1:]).all())
        got_rows = out["rows"][a].cpu().numpy()
        assert not got_rows[:, 3:].any() and np.array_equal(got_rows[:, :3], rows[rank.cpu().numpy()])
        left = torch.ones(full.numel(), dtype=torch.bool, device=full.device)
        if eligible is not None:
            left[:] = False
            left[eligible[a]] = True
            assert bool(left[rank].all())                                # no winner from outside the eligible ranks
        left[rank] = False
        assert float(full[left].max()) <= float(logit.min()) + 2e-6      # nobody left out beats the last winner


@pytest.mark.parametrize("chunk_rows", [999, 1 << 20])
def test_anchored_sweep_other_chromosome_d64(d64, trans, chunk_rows):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    out = SW.anchored_sweep(clf, trans["anchors"], lo, hi, 3, 3, top=100, chunk_rows=chunk_rows)
    assert out["n_candidates"] == 5 * 1035 and out["n_invalid"] == 0 and out["n_excluded"] == 0 and out["rows"].is_cuda
    check_trans_top(out, trans, 3, 100)
    assert torch.equal(out["proba"], torch.sigmoid(out["logit"]))
    wide = SW.anchored_sweep(clf, trans["anchors"], lo, hi, 3, 3, top=100, chunk_rows=chunk_rows, width=5)
    check_trans_top(wide, trans, 5, 100)
    for a in range(5):
        assert float((trans["full"][5][a] - trans["full"][3][a]).abs().max()) > 1e-4   # the width is part of the result (pads are attended)


def test_anchored_sweep_exclude_regress_empty_and_bad_ids(d64, trans):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    anchors, cf = trans["anchors"], trans["cf"]
    known = np.arange(0, cf, 7)                                          # every 7th candidate of every anchor (all are valid)
    hset = HyperedgeSet(torch.from_numpy(np.concatenate([rows[known] for rows in trans["rows"]])).cuda())
    everything = SW.anchored_sweep(clf, anchors, lo, hi, 3, 3, top=100)
    out = SW.anchored_sweep(clf, anchors, lo, hi, 3, 3, top=100, chunk_rows=999, exclude=hset)
    assert out["n_excluded"] == 5 * len(known) and out["n_invalid"] == 0 and out["n_candidates"] == 5 * cf
    assert not np.isin(out["rank"].cpu().numpy(), known).any()
    rest = torch.from_numpy(np.setdiff1d(np.arange(cf), known)).cuda()
    check_trans_top(out, trans, 3, 100, eligible=[rest] * 5)
    assert all(np.isin(everything["rank"][a].cpu().numpy(), known).any() for a in range(5))     # the exclusion did change the answer
    # an anchor inside the region: its invalid candidates are counted apart from the known ones, and neither is kept
    inside = np.asarray([lo + 10], dtype=np.int64)
    cand = [SW.anchored_unrank(r, inside.tolist(), lo, hi - lo, 3, 3) for r in range(cf)]
    valid = np.asarray([ok for _, ok in cand])
    some = np.flatnonzero(valid)[::7]
    rows_in = np.asarray([row for row, _ in cand], dtype=np.int64)
    mixed = HyperedgeSet(torch.from_numpy(np.concatenate([rows_in[some], rows_in[~valid][:3]])).cuda())
    got = SW.anchored_sweep(clf, inside, lo, hi, 3, 3, top=2000, exclude=mixed)
    assert got["n_invalid"] == int((~valid).sum()) > 0 and got["n_excluded"] == len(some)
    assert int(got["count"][0]) == int(valid.sum()) - len(some) and got["rows"].shape == (1, cf, 3)
    assert set(got["rank"][0, :int(got["count"][0])].tolist()) == set(np.flatnonzero(valid).tolist()) - set(some.tolist())
    reg = SW.anchored_sweep(clf, anchors, lo, hi, 3, 3, top=100, task_mode="regress")
    assert torch.equal(reg["rank"], everything["rank"]) and torch.equal(reg["proba"], torch.nn.functional.softplus(reg["logit"]))
    with pytest.raises(ValueError):
        SW.anchored_sweep(clf, anchors, lo, hi, 3, 3, top=100, task_mode="other")
    # no anchors, a region too small for two free nodes three apart, an empty region
    for table, region in ((anchors[:0], (lo, hi)), (anchors, (lo, lo + 3)), (anchors, (lo, lo))):
        with _lib.launch_log() as log:
            empty = SW.anchored_sweep(clf, table, *region, 3, 3, top=100)
        assert not log.counts and empty["n_candidates"] == 0 and empty["rows"].shape == (len(table), 0, 3)
        assert all(empty[key].shape == (len(table), 0) and empty[key].is_cuda for key in ("logit", "proba", "rank"))
        assert empty["count"].shape == (len(table),) and not empty["count"].any()
    with pytest.raises(IndexError):
        SW.anchored_sweep(clf, np.asarray([anchors[0], d64["N"] + 5]), lo, hi, 3, 3, top=10)     # an anchor beyond the model's table: once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    again = SW.anchored_sweep(clf, anchors, lo, hi, 3, 3, top=100)
    assert all(torch.equal(again[key], everything[key]) for key in ("rows", "logit", "proba", "rank", "count"))


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_anchored(tmp_path):
    num = R.FIXTURE_LAYOUTS["tiny"]
    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    node2bin, names = R.fixture_node2bin(num)
    np.save(os.path.join(temp, "node2bin.npy"), node2bin, allow_pickle=True)
    cr = np.asarray(synth.chrom_range(num))
    np.save(os.path.join(temp, "chrom_range.npy"), cr)
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": R.FIXTURE_RES, "chrom_list": names, "min_distance": 1}, f)
    bin2node = {v: key for key, v in node2bin.items()}

    def run(k, *extra):
        out = os.path.join(tmp_path, "anchored.tsv")
        PR.main(["anchored", "--chrom", "2", "--k", str(k), "--top", "6", "-o", out, "--config", cpath, *extra])
        z = np.load(os.path.join(tmp_path, "anchored.npz"))
        assert set(z.files) == {"anchors", "rows", "logit", "proba", "rank", "count"}
        lines = [line.rstrip("\n").split("\t") for line in open(out)]
        assert len(lines) == int(z["count"].sum())
        at = 0
        for a in range(len(z["anchors"])):                               # grouped by anchor, best first
            for row, p in zip(z["rows"][a, :z["count"][a]], z["proba"][a, :z["count"][a]]):
                assert [bin2node[item] for item in lines[at][:k]] == row.tolist() and np.float32(float(lines[at][k])) == p
                assert set(z["anchors"][a].tolist()) <= set(row.tolist())
                at += 1
        return z

    def same(z, ref):
        return all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in ("rows", "logit", "proba", "rank", "count"))

    clf = load_tiny("table")
    lo, hi = int(cr[2][0]), int(cr[2][1])
    # every bin of a window of chromosome 0 as a single anchor, partners on chromosome 2
    z = run(3, "--anchor-chrom", "0", "--anchor-start-bin", "2", "--anchor-end-bin", "7")
    a_lo = int(cr[0][0])
    anchors = np.arange(a_lo + 2, a_lo + 7, dtype=np.int64).reshape(-1, 1)
    assert np.array_equal(z["anchors"], anchors) and z["rows"].shape == (5, 6, 3) and (z["count"] == 6).all()
    assert same(z, SW.anchored_sweep(clf, anchors, lo, hi, 3, 2, top=6))                        # min_gap = min_distance + 1
    # two loci per line, one on chromosome 0 and one inside the partner window; positions anywhere inside their bins
    pairs = np.asarray([[a_lo + 1, lo + 4], [a_lo + 9, lo + 6], [lo + 5, lo + 9]], dtype=np.int64)
    apath = os.path.join(tmp_path, "loci.tsv")
    with open(apath, "w") as f:
        for p, q in pairs:
            (c1, s1), (c2, s2) = node2bin[int(p)].split(":"), node2bin[int(q)].split(":")
            f.write("%s:%d\t%s:%d\n" % (c2, int(s2) + R.FIXTURE_RES // 2, c1, int(s1) + 1))      # unsorted on the line
    w = run(4, "--anchor-file", apath, "--start-bin", "2", "--end-bin", "14")
    assert np.array_equal(w["anchors"], pairs)
    direct = SW.anchored_sweep(clf, pairs, lo + 2, lo + 14, 4, 2, top=6)
    assert same(w, direct) and direct["n_invalid"] > 0
    # --exclude-known drops the rows of all_3_counter.npy: each anchor's winners move up
    known = np.concatenate([z["rows"][0, [0, 3]], z["rows"][4, [1]]])
    np.save(os.path.join(temp, "all_3_counter.npy"), known)
    e = run(3, "--anchor-chrom", "0", "--anchor-start-bin", "2", "--anchor-end-bin", "7", "--exclude-known")
    more = SW.anchored_sweep(clf, anchors, lo, hi, 3, 2, top=8)["rows"].cpu().numpy()
    assert np.array_equal(e["rows"][0], more[0][[1, 2, 4, 5, 6, 7]]) and np.array_equal(e["rows"][4], more[4][[0, 2, 3, 4, 5, 6]])
    assert np.array_equal(e["rows"][1:4], more[1:4, :6])
