"""The de novo k-way sweep on the MI355X (csrc/sweep_rows.hip, csrc/sweep_select.hip, matcha_amd/sweep.py): candidate rows bit for bit against itertools and,
beyond 2^32, against kway_unrank; the streaming selection bit for bit against numpy's lexsort however the stream is cut; the sweep
against the reference's own logits (g11) and against one big batch of the d = 64 model; the CLI."""
import itertools
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
from tests.helpers import GOLD, gold, rel_err
from tests.test_cpu_kway import GRID, brute

pytestmark = pytest.mark.gpu

TOL = 1e-4                       # the device forward against the reference's CPU logits (test_predict_consumers.py)
SELECT_KERNELS = {"topk_keys_kernel", "topk_merge_kernel", "topk_commit_kernel"}


def rows_np(lo, n, k, g, width=None):
    ref = np.asarray(brute(lo, n, k, g), dtype=np.int64).reshape(-1, k)
    return np.pad(ref, ((0, 0), (0, (width or k) - k)))


# ---- rows, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo", [1, 3000])
@pytest.mark.parametrize("wide", [False, True])
def test_rows_grid_full_and_subranges(lo, wide):
    for n, k, g in GRID:
        width = 8 if wide else k
        ref = rows_np(lo, n, k, g, width)
        with _lib.launch_log() as log:
            got = SW.kway_rows(lo, n, k, g, width=width)
        assert got.shape == ref.shape and got.dtype == torch.long and np.array_equal(got.cpu().numpy(), ref), (n, k, g)
        assert (set(log.counts) == {"kway_rows_kernel"}) if len(ref) else not log.counts
        if len(ref) < 600:
            continue
        # ranges that start and end inside a run of rows sharing their first k - 1 nodes; counts around a wave and over a block
        same = (ref[1:, :k - 1] == ref[:-1, :k - 1]).all(axis=1)         # same[i]: rows i and i + 1 share the prefix
        for count in (1, 63, 64, 65, 300, 513):
            rank0 = next(r for r in range(3, len(ref) - count) if same[r - 1] and same[r + count - 1])
            got = SW.kway_rows(lo, n, k, g, rank0=rank0, count=count, width=width)
            assert np.array_equal(got.cpu().numpy(), ref[rank0:rank0 + count]), (n, k, g, rank0, count)


def test_rows_list_form_and_reused_buffer():
    lo, n, k, g = 7, 16, 4, 2
    ref = rows_np(lo, n, k, g, 6)
    total = len(ref)
    rng = np.random.default_rng(5)
    ranks = np.concatenate([rng.permutation(total), rng.integers(0, total, 300), [-1, total, total + 5, -(1 << 40), 1 << 62, 0, total - 1]])
    rng.shuffle(ranks)
    with _lib.launch_log() as log:
        got = SW.kway_rows(lo, n, k, g, ranks=torch.from_numpy(ranks).cuda(), width=6).cpu().numpy()
    assert log.counts == {"kway_rows_kernel": 1}                         # the same kernel as the range form
    ok = (ranks >= 0) & (ranks < total)
    assert np.array_equal(got[ok], ref[ranks[ok]]) and not got[~ok].any() and (~ok).sum() == 5
    # a region without candidates: every listed rank is out of range
    assert not SW.kway_rows(1, 6, 3, 3, ranks=torch.tensor([0, 1], device="cuda")).any()
    assert SW.kway_rows(1, 6, 3, 3).shape == (0, 3)
    # ``out`` reuses a caller's buffer and leaves its tail alone
    buf = torch.full((100 * 6,), -7, dtype=torch.long, device="cuda")
    x = SW.kway_rows(lo, n, k, g, rank0=10, count=40, width=6, out=buf)
    assert x.data_ptr() == buf.data_ptr() and np.array_equal(x.cpu().numpy(), ref[10:50]) and bool((buf[240:] == -7).all())


def test_rows_large_ranks_against_unrank():
    def check(n, k, g, rank0, count, lo=1):
        got = SW.kway_rows(lo, n, k, g, rank0=rank0, count=count).cpu().numpy()
        first = SW.kway_unrank(rank0, lo, n, k, g)
        assert tuple(got[0]) == first
        # successive rows: the lexicographic successor under the gap rule, checked row by row in numpy; the last row by unranking
        y = got - lo - np.arange(k) * (g - 1)
        m = n - (k - 1) * (g - 1)
        assert (np.diff(y, axis=1) > 0).all() and y.min() >= 0 and y.max() < m
        for a, b in zip(y[:-1], y[1:]):
            j = max(i for i in range(k) if a[i] < m - k + i)            # the last position that can still move
            assert np.array_equal(b[:j], a[:j]) and b[j] == a[j] + 1 and np.array_equal(b[j:], b[j] + np.arange(k - j))
        assert tuple(got[-1]) == SW.kway_unrank(rank0 + count - 1, lo, n, k, g)

    total = SW.kway_count(2491, 4, 1)
    assert total > 1 << 40
    check(2491, 4, 1, 1 << 40, 1000)
    check(2491, 4, 1, total - 1000, 1000)
    check(2491, 4, 2, total // 7, 1000, lo=3000)
    total = SW.kway_count(250, 8, 1)
    check(250, 8, 1, total - 100, 100)
    # n = 120 000, k = 4: C(m, k) > 2^62, where C(a, j - 1) (a - j + 1) passes 2^64 before the division
    n, k, g = 120000, 4, 1
    total = SW.kway_count(n, k, g)
    assert total > 1 << 62
    ranks = [0, total // 2 - 3, total // 2, total // 2 + 3, total - 1]
    got = SW.kway_rows(1, n, k, g, ranks=torch.tensor(ranks, device="cuda")).cpu().numpy()
    for r, row in zip(ranks, got):
        assert tuple(row) == SW.kway_unrank(r, 1, n, k, g), r
    assert tuple(SW.kway_rows(1, n, k, g, rank0=total - 1, count=1).cpu().numpy()[0]) == (n - 3, n - 2, n - 1, n)
    with pytest.raises(IndexError):
        SW.kway_rows(1, n, k, g, rank0=total - 1, count=2)


# ---- selection, exact, no model ----------------------------------------------------------------------------------------------------
def salted_scores(n=100000, seed=11):
    """Seeded scores quantised to 257 values (ties abound), salted with +-inf, NaN, -0.0 / +0.0 pairs, and a skip mask."""
    rng = np.random.default_rng(seed)
    s = (np.round(rng.standard_normal(n) * 40.0).clip(-128, 128) / 16.0).astype(np.float32)
    assert n < 100000 or len(np.unique(s)) == 257
    for value, count in ((np.inf, 5), (-np.inf, 5), (np.nan, 50), (-0.0, 400), (0.0, 400)):
        s[rng.choice(n, count, replace=False)] = value
    skip = (rng.random(n) < 0.1).astype(np.int32) * rng.integers(1, 5, n).astype(np.int32)   # any non-zero value skips
    assert np.isnan(s).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    return s, skip


def lexsort_ref(s, skip, K, rank0=0):
    valid = np.flatnonzero(~np.isnan(s) & (skip == 0))
    order = valid[np.lexsort((valid, -s[valid]))][:K]                    # higher score first (-0.0 == +0.0), then lower rank
    return s[order], order.astype(np.int64) + rank0


def run_topk(s, skip, K, piece, rank0=0):
    sel = SW.TopK(K, piece, "cuda")
    st, kt = torch.from_numpy(s).cuda(), torch.from_numpy(skip).cuda()
    for a in range(0, len(s), piece):
        sel.update(st[a:a + piece], rank0 + a, kt[a:a + piece])
    sc, rk = sel.result()
    return sc.cpu().numpy(), rk.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("K", [1, 7, 64, 1000, 4096, 65536])
def test_selection_exact_however_the_stream_is_cut(K):
    s, skip = salted_scores()
    rank0 = (1 << 40) + 3
    ref_s, ref_r = lexsort_ref(s, skip, K, rank0)
    assert len(ref_s) == min(K, int((~np.isnan(s) & (skip == 0)).sum()))
    for piece in (37, 64, 4099, len(s)):
        got_s, got_r = run_topk(s, skip, K, piece, rank0)
        assert np.array_equal(got_r, ref_r), (K, piece)
        assert same_bits(got_s, ref_s), (K, piece)                       # the kept score keeps its bits (-0.0 stays -0.0)
    # single-row updates, on the first 300 rows
    ref_s, ref_r = lexsort_ref(s[:300], skip[:300], K)
    for piece in (1, 300):
        got_s, got_r = run_topk(s[:300], skip[:300], K, piece)
        assert np.array_equal(got_r, ref_r) and same_bits(got_s, ref_s), (K, piece)


def test_selection_order_of_special_values():
    s = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -0.0, 0.0, np.inf, -1.0, np.nan, -np.inf], dtype=np.float32)
    got_s, got_r = run_topk(s, np.zeros(len(s), dtype=np.int32), 64, 5)
    assert list(got_r) == [2, 8, 5, 0, 1, 6, 7, 9, 3, 11]                # +inf first, zeros by rank whatever their sign, -inf last, no NaN
    assert same_bits(got_s, s[got_r])
    got_s, got_r = run_topk(s, (np.arange(len(s)) % 2).astype(np.int32), 3, 12)
    assert list(got_r) == [2, 8, 0]


def test_selection_fewer_valid_rows_than_k_and_empty_updates():
    rng = np.random.default_rng(2)
    s = rng.standard_normal(50).astype(np.float32)
    s[rng.choice(50, 5, replace=False)] = np.nan
    ref_s, ref_r = lexsort_ref(s, np.zeros(50, dtype=np.int32), 64)
    assert len(ref_r) == 45
    sel = SW.TopK(64, 50, "cuda")
    assert sel.result()[0].numel() == 0 and sel.result()[1].numel() == 0   # nothing seen yet
    with _lib.launch_log() as log:
        sel.update(torch.zeros(0, device="cuda"), 0)                     # an empty update launches nothing
    assert not log.counts
    with _lib.launch_log() as log:
        sel.update(torch.from_numpy(s).cuda(), 0)
        sel.update(torch.zeros(0, device="cuda"), 50)
        sc, rk, cnt = sel.read()
    assert set(log.counts) == SELECT_KERNELS | {"topk_read_kernel"} and all(v == 1 for v in log.counts.values())
    assert int(cnt) == 45 and np.array_equal(rk[:45].cpu().numpy(), ref_r) and same_bits(sc[:45].cpu().numpy(), ref_s)
    assert bool((rk[45:] == -1).all())
    with pytest.raises(_lib.MatchaHipError):
        sel.update(torch.zeros(51, device="cuda"), 0)                    # more rows than max_chunk
    with pytest.raises(ValueError):
        SW.TopK(0, 10, "cuda")


def test_two_selections_alive_at_once():
    s, skip = salted_scores(5000, seed=3)
    t = np.random.default_rng(4).standard_normal(5000).astype(np.float32)
    none = np.zeros(5000, dtype=np.int32)
    a, b = SW.TopK(100, 512, "cuda"), SW.TopK(7, 700, "cuda")
    st, kt, tt = torch.from_numpy(s).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(t).cuda()
    pa = pb = 0
    while pa < 5000 or pb < 5000:                                        # interleaved updates of different sizes
        if pa < 5000:
            a.update(st[pa:pa + 512], pa, kt[pa:pa + 512])
            pa += 512
        if pb < 5000:
            b.update(tt[pb:pb + 700], pb)
            pb += 700
    for sel, (ref_s, ref_r) in ((a, lexsort_ref(s, skip, 100)), (b, lexsort_ref(t, none, 7))):
        sc, rk = sel.result()
        assert np.array_equal(rk.cpu().numpy(), ref_r) and same_bits(sc.cpu().numpy(), ref_s)


# ---- against the reference ---------------------------------------------------------------------------------------------------------
def load_tiny(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    return torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False)


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_sweep_against_reference_logits(mode):
    g = gold("g11_kway_tiny.npz")
    clf = load_tiny(mode)
    cr = np.asarray(synth.chrom_range([int(v) for v in g["num"]]))
    for i, (c, k, gap) in enumerate(g["cases"]):
        c, k, gap = int(c), int(k), int(gap)
        lo, hi = int(cr[c][0]), int(cr[c][1])
        rows, ref = g[f"rows_c{i}"], g[f"logit_{mode}_c{i}"]
        with _lib.launch_log() as log:
            out = SW.kway_sweep(clf, lo, hi, k, gap, top=len(rows))
        assert {"kway_rows_kernel", "topk_init_kernel", "topk_read_kernel"} | SELECT_KERNELS <= set(log.counts)
        assert log.counts["kway_rows_kernel"] == 2 and log.counts["topk_merge_kernel"] == 1      # one chunk, then the winners' rows
        assert out["n_candidates"] == len(rows) and out["n_excluded"] == 0
        rank = out["rank"].cpu().numpy()
        assert np.array_equal(np.sort(rank), np.arange(len(rows)))       # every candidate once
        assert np.array_equal(out["rows"].cpu().numpy(), rows[rank])
        by_rank = np.empty(len(rows), dtype=np.float32)
        by_rank[rank] = out["logit"].cpu().numpy()
        assert rel_err(by_rank, ref) < TOL
        assert torch.equal(out["proba"], torch.sigmoid(out["logit"])) and bool((out["logit"][:-1] >= out["logit"][1:]).all())
        K = int(g[f"ksel_{mode}_c{i}"])
        want = set(np.argsort(-ref.astype(np.float64))[:K].tolist())
        for chunk_rows in (37, 10000):
            top = SW.kway_sweep(clf, lo, hi, k, gap, top=K, chunk_rows=chunk_rows)
            assert set(top["rank"].cpu().numpy().tolist()) == want, (i, chunk_rows)
            assert np.array_equal(top["rows"].cpu().numpy(), rows[top["rank"].cpu().numpy()])


# ---- at d = 64 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d64():
    """The d = 64 table model of test_pairwise_sweep_full_chromosome_properties, the 48-bin chromosome of hg38 at 1 Mb, k = 3,
    min_gap = 3: 13 244 candidates, their rows, and ``full`` = model(all rows) in one batch at widths 3 and 5."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    c = num.index(48)
    cr = np.asarray(synth.chrom_range(num))
    lo, hi = int(cr[c][0]), int(cr[c][1])
    clf, _ = hip_model(num, 64, "table", 12)
    clf.eval()
    rows = rows_np(lo, hi - lo, 3, 3)
    assert len(rows) == 13244 == SW.kway_count(48, 3, 3)
    full = {}
    with torch.no_grad():
        for width in (3, 5):
            x = torch.from_numpy(np.pad(rows, ((0, 0), (0, width - 3)))).cuda()
            full[width] = clf(x).reshape(-1).clone()
    return dict(clf=clf, lo=lo, hi=hi, rows=rows, full=full, N=int(np.sum(num)))


def check_top(out, full, rows, lo, n, width, candidates=None, top=100):
    """The properties of a sweep result against ``full`` (logits of every candidate, by rank); ``candidates``: the ranks that were
    eligible (default all)."""
    rank = out["rank"]
    assert rank.numel() == top and len(set(rank.tolist())) == top
    assert float((out["logit"] - full[rank]).abs().max()) <= 1e-6        # what two batchings of one forward may differ by
    assert bool((out["logit"][:-1] >= out["logit"][1:]).all())
    got_rows = out["rows"].cpu().numpy()
    assert got_rows.shape == (top, width) and not got_rows[:, 3:].any()
    for r, row in zip(rank.tolist()[::9], got_rows[::9]):
        assert tuple(row[:3]) == SW.kway_unrank(r, lo, n, 3, 3)
    assert np.array_equal(got_rows[:, :3], rows[rank.cpu().numpy()])
    left = torch.ones(full.numel(), dtype=torch.bool, device=full.device)
    if candidates is not None:
        left[:] = False
        left[candidates] = True
        assert bool(left[rank].all())                                    # no winner from outside the eligible ranks
    left[rank] = False
    assert float(full[left].max()) <= float(out["logit"].min()) + 2e-6   # nobody left out beats the last winner


@pytest.mark.parametrize("chunk_rows", [4099, 1 << 20])
def test_sweep_d64_properties(d64, chunk_rows):
    n = d64["hi"] - d64["lo"]
    out = SW.kway_sweep(d64["clf"], d64["lo"], d64["hi"], 3, 3, top=100, chunk_rows=chunk_rows)
    assert out["n_candidates"] == 13244 and out["n_excluded"] == 0 and out["rows"].is_cuda
    check_top(out, d64["full"][3], d64["rows"], d64["lo"], n, 3)
    assert torch.equal(out["proba"], torch.sigmoid(out["logit"]))
    wide = SW.kway_sweep(d64["clf"], d64["lo"], d64["hi"], 3, 3, top=100, chunk_rows=chunk_rows, width=5)
    check_top(wide, d64["full"][5], d64["rows"], d64["lo"], n, 5)
    assert float((d64["full"][5] - d64["full"][3]).abs().max()) > 1e-4   # the width is part of the result (pads are attended)


def test_sweep_d64_exclude_regress_empty_and_bad_region(d64):
    clf, lo, hi, rows = d64["clf"], d64["lo"], d64["hi"], d64["rows"]
    n = hi - lo
    known = np.arange(0, len(rows), 7)
    hset = HyperedgeSet(torch.from_numpy(np.pad(rows[known], ((0, 0), (0, 2)))).cuda())      # known hyperedges, padded to L = 5
    out = SW.kway_sweep(clf, lo, hi, 3, 3, top=100, chunk_rows=4099, exclude=hset)
    assert out["n_excluded"] == len(known) and out["n_candidates"] == 13244
    assert not np.isin(out["rank"].cpu().numpy(), known).any()
    rest = np.setdiff1d(np.arange(len(rows)), known)
    check_top(out, d64["full"][3], rows, lo, n, 3, candidates=torch.from_numpy(rest).cuda())
    everything = SW.kway_sweep(clf, lo, hi, 3, 3, top=100)
    assert np.isin(everything["rank"].cpu().numpy(), known).any()        # the exclusion did change the answer
    # top larger than what is left: everything that is not excluded, once
    tiny = SW.kway_sweep(clf, lo, lo + 9, 3, 3, top=1000, exclude=hset)
    assert tiny["n_candidates"] == 10 and tiny["rank"].numel() == 10 - tiny["n_excluded"] and tiny["n_excluded"] >= 1
    reg = SW.kway_sweep(clf, lo, hi, 3, 3, top=100, task_mode="regress")
    assert torch.equal(reg["rank"], everything["rank"]) and torch.equal(reg["proba"], torch.nn.functional.softplus(reg["logit"]))
    with pytest.raises(ValueError):
        SW.kway_sweep(clf, lo, hi, 3, 3, top=100, task_mode="other")
    with _lib.launch_log() as log:
        empty = SW.kway_sweep(clf, lo, lo + 6, 3, 3, top=100)            # n = 6, k = 3, min_gap = 3: no candidates
    assert not log.counts and empty["n_candidates"] == 0 and empty["rows"].shape == (0, 3)
    assert all(empty[key].numel() == 0 and empty[key].is_cuda for key in ("logit", "proba", "rank"))
    with pytest.raises(IndexError):
        SW.kway_sweep(clf, d64["N"] - 10, d64["N"] + 10, 3, 3, top=10)   # a region beyond the model's table: raised once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    again = SW.kway_sweep(clf, lo, hi, 3, 3, top=100)
    assert torch.equal(again["rank"], everything["rank"]) and torch.equal(again["logit"], everything["logit"])


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_kway(tmp_path):
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

    def run(*extra):
        out = os.path.join(tmp_path, "top.tsv")
        PR.main(["kway", "--chrom", "2", "--k", "3", "--top", "20", "-o", out, "--config", cpath, *extra])
        z = np.load(os.path.join(tmp_path, "top.npz"))
        lines = [line.rstrip("\n").split("\t") for line in open(out)]
        assert len(lines) == len(z["rows"]) and set(z.files) == {"rows", "logit", "proba", "rank"}
        bin2node = {v: k for k, v in node2bin.items()}
        for line, row, p in zip(lines, z["rows"], z["proba"]):
            assert [bin2node[item] for item in line[:3]] == row.tolist() and all(item.startswith("chr3:") for item in line[:3])
            assert np.float32(float(line[3])) == p
        return z

    z = run()
    lo, hi = int(cr[2][0]), int(cr[2][1])
    clf = load_tiny("table")
    ref = SW.kway_sweep(clf, lo, hi, 3, 2, top=20)                       # min_gap = min_distance + 1
    assert np.array_equal(z["rank"], ref["rank"].cpu().numpy()) and np.array_equal(z["rows"], ref["rows"].cpu().numpy())
    assert all(tuple(r) == SW.kway_unrank(int(q), lo, hi - lo, 3, 2) for r, q in zip(z["rows"], z["rank"]))
    # a window of bins inside the chromosome
    w = run("--start-bin", "2", "--end-bin", "12")
    assert w["rows"].min() >= lo + 2 and w["rows"].max() < lo + 12
    # --exclude-known drops the rows of all_3_counter.npy: the winners move up
    known = z["rows"][[0, 3, 4]]
    np.save(os.path.join(temp, "all_3_counter.npy"), known)
    e = run("--exclude-known")
    more = SW.kway_sweep(clf, lo, hi, 3, 2, top=23)["rows"].cpu().numpy()
    keep = [i for i in range(23) if i not in (0, 3, 4)]
    assert np.array_equal(e["rows"], more[keep])
