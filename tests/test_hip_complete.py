"""Cluster completion on the MI355X (csrc/sweep_rows.hip's kway_complete_rows_kernel, matcha_amd/sweep.py): candidate rows and
flags bit for bit against the itertools twin (tests/complete_ref.py) and against the anchored kernel; the sweep against the reference's
own logits per cluster (g15), independent of how it is cut; exclusion, errors and empty cases; the untouched sweeps; the CLI."""
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
from tests import complete_ref as CR
from tests import denoise_ref as R
from tests.helpers import GOLD, gold, logit_err
from tests.test_cpu_complete import g15_case
from tests.test_hip_kway import SELECT_KERNELS, load_tiny
from tests.test_hip_long_rows import LONG, SHORT_ONLY

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
KERNEL = "kway_complete_rows_kernel"
SEG_KERNELS = {"segtopk_keys_kernel", "segtopk_merge_kernel", "segtopk_commit_kernel"}
KEYS = ("rows", "logit", "proba", "rank", "count", "added")


def got_np(pair):
    x, flag = pair
    assert x.dtype == torch.long and flag.dtype == torch.int32 and flag.shape == (x.shape[0],)
    return x.cpu().numpy(), flag.cpu().numpy() != 0


def region(f, g):
    """(lo, n): 16 nodes, or what a free part of 8 needs to have candidates (495 at min_gap 1, 45 at min_gap 3)."""
    return (5, 16) if f < 8 else (5, 12 if g == 1 else 24)


def mixed_table(rng, S, lo, n):
    """Clusters with s_a = 0, 1, S - 1 and S in one table [A, S]: ids inside the region (a free id meets a cluster id), around it and
    far above; one row that repeats an id."""
    pool = np.arange(1, 3 * (lo + n))
    sizes = sorted({0, 1, max(S - 1, 1), S, min(S, 3)})
    clusters = [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s in sizes]
    clusters.append([lo + 2])                                            # a single id inside the region
    if S >= 2:
        clusters.append(sorted([lo + 3, lo + 3] + [int(v) for v in rng.choice(pool, size=min(S, 4) - 2, replace=False)]))
    return clusters


# ---- rows and flags, exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 8, 9, 31])
def test_rows_grid(S):
    rng = np.random.default_rng(100 + S)
    seen = set()
    for f in (1, 2, 8):
        if S + f > 32:
            continue
        for g in (1, 3):
            lo, n = region(f, g)
            clusters = mixed_table(rng, S, lo, n)
            table = CR.padded(clusters, S)
            for L in sorted({S + f, 32}):
                ref, bad = CR.table(clusters, lo, n, f, g, L)
                assert len(ref) == len(clusters) * SW.completion_count(1, S, n, f, g) > 0
                with _lib.launch_log() as log:
                    x, inv = got_np(SW.completion_rows(table, lo, n, f, g, width=L))
                assert x.shape == ref.shape and np.array_equal(x, ref) and np.array_equal(inv, bad), (S, f, g, L)
                assert log.counts == {KERNEL: 1}                         # it, and only it
                assert bad.any() and not bad.all()
                seen.add((f, g, L == 32))
            # the same clusters as id lists of different lengths: the wrapper pads them
            x2, inv2 = got_np(SW.completion_rows(clusters, lo, n, f, g, width=32))
            assert np.array_equal(x2, ref) and np.array_equal(inv2, bad)
    assert (1, 3, True) in seen and ((1, 1, False) in seen) == (S < 31) and ((8, 3, True) in seen) == (S + 8 <= 32)


def test_rows_ranges_counts_and_rank_lists():
    """40 clusters of 0 .. 9 ids, two free nodes of [5, 21): 4 800 ranks.  Ranges that begin and end inside a cluster's segment, counts
    around a wavefront and over many blocks, a rank list with out-of-range and repeated entries, reused buffers."""
    lo, n, f, g, S, L = 5, 16, 2, 1, 9, 12
    rng = np.random.default_rng(7)
    clusters = [sorted(int(v) for v in rng.choice(np.arange(1, 60), size=int(s), replace=False)) for s in rng.integers(0, S + 1, size=40)]
    clusters[3], clusters[17] = list(range(2, 2 + S)), []
    ref, bad = CR.table(clusters, lo, n, f, g, L)
    cf = 120
    assert len(ref) == 40 * cf == SW.completion_count(40, S, n, f, g)
    table = torch.from_numpy(CR.padded(clusters, S)).cuda()
    for count in (1, 63, 64, 65, 4099):
        for rank0 in (0, 3 * cf + 41, len(ref) - count):
            x, inv = got_np(SW.completion_rows(table, lo, n, f, g, rank0=rank0, count=count, width=L))
            assert np.array_equal(x, ref[rank0:rank0 + count]) and np.array_equal(inv, bad[rank0:rank0 + count]), (rank0, count)
    with pytest.raises(IndexError):
        SW.completion_rows(table, lo, n, f, g, rank0=len(ref) - 1, count=2, width=L)
    total = len(ref)
    ranks = np.concatenate([rng.permutation(total)[:700], rng.integers(0, total, 300), [-1, total, 1 << 62, -(1 << 40), 0, 0, total - 1]])
    rng.shuffle(ranks)
    with _lib.launch_log() as log:
        x, inv = got_np(SW.completion_rows(table, lo, n, f, g, ranks=torch.from_numpy(ranks).cuda(), width=L))
    assert log.counts == {KERNEL: 1}                                     # the same kernel as the range form
    ok = (ranks >= 0) & (ranks < total)
    assert np.array_equal(x[ok], ref[ranks[ok]]) and np.array_equal(inv[ok], bad[ranks[ok]])
    assert not x[~ok].any() and inv[~ok].all() and (~ok).sum() == 4      # out of range: a zero row with its flag set
    # no clusters, or a region without candidates: every listed rank is out of range, and the range form is empty
    for tab, reg in ((np.zeros((0, 3), dtype=np.int64), (lo, n)), (CR.padded(clusters, S), (1, 1))):
        x, inv = got_np(SW.completion_rows(tab, *reg, f, g, ranks=torch.tensor([0, 1], device="cuda")))
        assert not x.any() and inv.all()
        with _lib.launch_log() as log:
            assert SW.completion_rows(tab, *reg, f, g, device="cuda")[0].shape[0] == 0
        assert not log.counts
    buf = torch.full((100 * L,), -7, dtype=torch.long, device="cuda")
    fbuf = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    x, flag = SW.completion_rows(table, lo, n, f, g, rank0=130, count=40, width=L, out=buf, flag_out=fbuf)
    assert x.data_ptr() == buf.data_ptr() and flag.data_ptr() == fbuf.data_ptr()
    assert np.array_equal(x.cpu().numpy(), ref[130:170]) and np.array_equal(flag.cpu().numpy() != 0, bad[130:170])
    assert bool((buf[40 * L:] == -7).all()) and bool((fbuf[40:] == -7).all())


def test_c_contract_reads_the_leading_run_and_flags_a_descending_row():
    """Tables handed straight to the C entry point, as they stand: ids behind the first zero are ignored; a row that descends somewhere
    leaves unmerged with every flag set; the wrapper sorts the same rows first."""
    lo, n, f, g, S, L = 5, 16, 2, 1, 6, 9
    raw = [[40, 7, 9, 0, 0, 0], [3, 9, 0, 50, 2, 0], [0, 8, 9, 0, 0, 0], [7, 7, 12, 30, 0, 0], [2, 6, 10, 11, 25, 4], [1, 2, 3, 4, 5, 6]]
    table = torch.tensor(raw, dtype=torch.long, device="cuda")
    ref, bad = CR.table(raw, lo, n, f, g, L)
    x, inv = got_np(SW._complete_rows(table, lo, n, f, g, 0, None, None, L, None, None))
    assert np.array_equal(x, ref) and np.array_equal(inv, bad)
    cf = 120
    assert bad[:cf].all() and np.array_equal(ref[0, :5], [40, 7, 9, 5, 6])               # descending: unmerged, flagged
    assert np.array_equal(ref[cf, :5], [3, 5, 6, 9, 0]) and not bad[cf:2 * cf].all()      # [3, 9]: what stands behind the zero is ignored
    assert bad[2 * cf:3 * cf].all() and np.array_equal(ref[2 * cf, :3], [5, 6, 0])        # no leading id: the free part alone, flagged
    assert bad[3 * cf:4 * cf].all() and bad[4 * cf:5 * cf].all()                         # a repeated id; a descent at the last id
    xs, invs = got_np(SW.completion_rows(raw, lo, n, f, g, width=L))                      # the wrapper: every row sorted, zeros last
    srt = [sorted(v for v in r if v) for r in raw]
    ref_s, bad_s = CR.table(srt, lo, n, f, g, L)
    assert np.array_equal(xs, ref_s) and np.array_equal(invs, bad_s) and not bad_s[:cf].all() and not bad_s[4 * cf:5 * cf].all()


@pytest.mark.parametrize("s,f,g", [(1, 1, 1), (1, 2, 2), (2, 2, 3), (3, 1, 1), (5, 3, 1), (7, 1, 2)])
def test_rows_equal_the_anchored_kernel(s, f, g):
    lo, n, k = 5, 16, s + f
    anchors = np.asarray([[a + 4 * j for j in range(s)] for a in range(1, 31)], dtype=np.int64)
    for width in sorted({k, 8}):
        with _lib.launch_log() as log:
            xa, fa = SW.anchored_rows(anchors, lo, n, k, g, width=width)
        assert set(log.counts) == {"kway_anchor_rows_kernel"}
        with _lib.launch_log() as log:
            xc, fc = SW.completion_rows(anchors, lo, n, f, g, width=width)
        assert set(log.counts) == {KERNEL}
        assert xa.shape[0] == 30 * SW.anchored_count(1, s, n, k, g) > 0
        assert torch.equal(xa, xc) and torch.equal(fa != 0, fc != 0) and bool(fa.any()) and not bool(fa.all())


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_completion_sweep_against_reference_logits(mode):
    g = gold("g15_complete_tiny.npz")
    clf = load_tiny(mode)
    for i in range(len(CR.G15_CASES)):
        clusters, lo, n, free, gap, W = g15_case(g, i)
        rows, valid = g[f"rows_c{i}"].astype(np.int64), g[f"valid_c{i}"]
        ref, ksel = g[f"logit_{mode}_c{i}"].astype(np.float64), g[f"ksel_{mode}_c{i}"]
        A, cf = len(clusters), len(rows) // len(clusters)
        top = 8                                                          # the largest K_a there can be; cut per cluster below
        with _lib.launch_log() as log:
            out = SW.completion_sweep(clf, clusters, lo, lo + n, free=free, min_gap=gap, top=top, width=W)
        ran = {name for name, c in log.counts.items() if c > 0}
        assert LONG <= ran and not (ran & SHORT_ONLY), sorted(ran)       # widths 9, 16 and 32: the long plan and attention
        assert not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)                 # no training kernel
        assert log.counts[KERNEL] == 3 and log.counts["segtopk_merge_kernel"] == 1 and "kway_anchor_rows_kernel" not in ran
        assert out["n_candidates"] == len(rows) == A * cf and out["n_invalid"] == int((~valid).sum()) and out["n_excluded"] == 0
        assert out["rows"].shape == (A, top, W) and out["added"].shape == (A, top, free) and out["logit"].shape == (A, top)
        for a in range(A):
            ok = np.flatnonzero(valid[a * cf:(a + 1) * cf])
            assert int(out["count"][a]) == min(top, len(ok))
            K = int(ksel[a])
            rank = out["rank"][a, :K].cpu().numpy()
            assert np.isin(rank, ok).all() and len(set(rank.tolist())) == K
            logit = out["logit"][a, :K].cpu().numpy()
            e = logit_err(logit, ref[a * cf + rank])
            assert e <= TOL, (mode, i, a, e)
            assert set(rank.tolist()) == set(ok[np.argsort(-ref[a * cf + ok])[:K]].tolist()), (mode, i, a)     # the reference's top K_a
            count = int(out["count"][a])
            kept_rows = out["rows"][a, :count].cpu().numpy()
            assert np.array_equal(kept_rows, rows[a * cf + out["rank"][a, :count].cpu().numpy()])
            for row, add, r in zip(kept_rows.tolist(), out["added"][a, :count].tolist(), out["rank"][a, :count].tolist()):
                assert sorted(clusters[a] + add) == [v for v in row if v] and tuple(add) == CR.free_parts(lo, n, free, gap)[r]
                assert SW.completion_unrank(r, clusters[a], lo, n, free, gap) == (tuple(v for v in row if v), True)
            assert bool((out["rank"][a, count:] == -1).all()) and not out["rows"][a, count:].any() and not out["added"][a, count:].any()
            assert not out["logit"][a, count:].any() and not out["proba"][a, count:].any()
        kept = out["rank"] >= 0
        assert torch.equal(out["proba"][kept], torch.sigmoid(out["logit"][kept]))
        for chunk_rows in (37, 4099):                                    # the cut is not part of the result
            again = SW.completion_sweep(clf, clusters, lo, lo + n, free=free, min_gap=gap, top=top, width=W, chunk_rows=chunk_rows)
            assert all(torch.equal(again[key], out[key]) for key in KEYS), (mode, i, chunk_rows)


@pytest.fixture(scope="module")
def d64():
    """The d = 64 table model of tests/test_hip_kway.py on hg38 at 1 Mb; the 48-bin chromosome is the partner region."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    cr = np.asarray(synth.chrom_range(num))
    c = num.index(48)
    clf, _ = hip_model(num, 64, "table", 12)
    return dict(clf=clf.eval(), lo=int(cr[c][0]), hi=int(cr[c][1]), N=int(np.sum(num)), chr1=(int(cr[0][0]), int(cr[0][1])))


def d64_clusters(d64, rng, sizes):
    """Clusters across chromosome 1 and the partner chromosome."""
    pool = np.concatenate([np.arange(*d64["chr1"]), np.arange(d64["lo"], d64["hi"])])
    return [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s in sizes]


def test_sweep_does_not_depend_on_the_cut_d64(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    rng = np.random.default_rng(21)
    wide = d64_clusters(d64, rng, [9, 25, 12, 17, 1, 20, 24, 10])       # width 27, two free nodes: 8 x 1 128 rows, the long forward
    short = d64_clusters(d64, rng, [1, 6, 3, 5, 2, 6, 4, 1])            # up to width 8: the L <= 8 forward, ragged clusters
    for clusters, free, width, long_rows in ((wide, 2, None, True), (wide, 1, 32, True), (short, 1, 8, False), (short, 2, None, False)):
        first = None
        for chunk_rows in (None, 37, 4099):
            with _lib.launch_log() as log:
                out = SW.completion_sweep(clf, clusters, lo, hi, free=free, min_gap=1, top=50, width=width, chunk_rows=chunk_rows)
            ran = {name for name, c in log.counts.items() if c > 0}
            assert (LONG <= ran and not (ran & SHORT_ONLY)) if long_rows else (ran & SHORT_ONLY and not (ran & LONG)), sorted(ran)
            assert not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)
            if first is None:
                first = out
                assert out["rows"].shape[2] == (width or max(len(c) for c in clusters) + free) and bool((out["count"] > 0).all())
                assert out["n_invalid"] > 0
            else:
                assert all(torch.equal(out[key], first[key]) for key in KEYS), (free, width, chunk_rows)
                assert (out["n_candidates"], out["n_invalid"]) == (first["n_candidates"], first["n_invalid"])
        # the kept logits are model(x)'s on the kept rows, on the same route
        with torch.no_grad(), _lib.option("disable_small_batch"):
            direct = clf(first["rows"].view(-1, first["rows"].shape[2])).view(first["logit"].shape)
        kept = first["rank"] >= 0
        assert float((direct[kept] - first["logit"][kept]).abs().max()) <= 1e-6     # what two batchings of one forward may differ by


def test_exclude_counts_and_kept_ranks(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    n, free, gap = hi - lo, 1, 3
    clusters = d64_clusters(d64, np.random.default_rng(5), [12, 25, 9, 1])
    ref, bad = CR.table(clusters, lo, n, free, gap, 32)
    cf = n
    assert bad.any() and not bad.all()
    known = np.concatenate([np.flatnonzero(~bad)[::5], np.flatnonzero(bad)[::3]])      # some valid and some invalid candidates
    hset = HyperedgeSet(torch.from_numpy(ref[known]).cuda())
    assert hset.L == 32
    out = SW.completion_sweep(clf, clusters, lo, hi, free=free, min_gap=gap, top=cf, width=32, exclude=hset, chunk_rows=50)
    n_known_valid = len(np.flatnonzero(~bad)[::5])
    assert out["n_excluded"] == n_known_valid and out["n_invalid"] == int(bad.sum()) and out["n_candidates"] == len(ref)
    left = ~bad
    left[known] = False
    for a in range(len(clusters)):
        want = np.flatnonzero(left[a * cf:(a + 1) * cf])
        assert int(out["count"][a]) == len(want)
        assert set(out["rank"][a, :len(want)].tolist()) == set(want.tolist()) and bool((out["rank"][a, len(want):] == -1).all())
    everything = SW.completion_sweep(clf, clusters, lo, hi, free=free, min_gap=gap, top=cf, width=32)
    assert everything["n_excluded"] == 0 and int(everything["count"].sum()) == int((~bad).sum())
    reg = SW.completion_sweep(clf, clusters, lo, hi, free=free, min_gap=gap, top=cf, width=32, task_mode="regress")
    assert torch.equal(reg["rank"], everything["rank"]) and torch.equal(reg["proba"][reg["rank"] >= 0],
                                                                        torch.nn.functional.softplus(reg["logit"][reg["rank"] >= 0]))


def test_errors_and_empty_cases(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    clusters = d64_clusters(d64, np.random.default_rng(6), [12, 3])
    clf._runtime()                                                       # (packing the model's parameters is not the sweep's doing)
    with _lib.launch_log() as log:
        for kw in (dict(width=33), dict(width=12), dict(free=9), dict(free=0), dict(width=32, chunk_rows=1 << 27), dict(top=0),
                   dict(task_mode="other")):
            with pytest.raises(ValueError):
                SW.completion_sweep(clf, clusters, lo, hi, **kw)
        with pytest.raises(ValueError):
            SW.completion_sweep(clf, [list(range(1, 33))], lo, hi)       # a cluster of 32 ids
        with pytest.raises(ValueError):
            SW.completion_sweep(clf, [list(range(1, 31))], lo, hi, free=3)
        # no clusters, a region too small for the free part, an empty region
        for tab, reg, free in (([], (lo, hi), 1), (clusters, (lo, lo + 3), 2), (clusters, (lo, lo), 1)):
            empty = SW.completion_sweep(clf, tab, *reg, free=free, min_gap=3)
            W = (12 if tab else 1) + free
            assert empty["n_candidates"] == 0 and empty["rows"].shape == (len(tab), 0, W) and empty["added"].shape == (len(tab), 0, free)
            assert all(empty[key].shape == (len(tab), 0) and empty[key].is_cuda for key in ("logit", "proba", "rank"))
            assert empty["count"].shape == (len(tab),) and not empty["count"].any()
    assert not log.counts
    with pytest.raises(IndexError):
        SW.completion_sweep(clf, [clusters[0], [3, d64["N"] + 5]], lo, hi)      # a cluster id beyond the model's table: once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    a, b = SW.completion_sweep(clf, clusters, lo, hi, top=5), SW.completion_sweep(clf, clusters, lo, hi, top=5)
    assert all(torch.equal(a[key], b[key]) for key in KEYS) and a["rows"].shape == (2, 5, 13)


def test_the_other_sweeps_launch_what_they_launched(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    with _lib.launch_log() as log:
        SW.anchored_sweep(clf, np.asarray([d64["chr1"][0], d64["chr1"][0] + 9]), lo, hi, 3, 3, top=10, chunk_rows=999)
    assert {"kway_anchor_rows_kernel", "segtopk_init_kernel", "segtopk_read_kernel"} | SEG_KERNELS <= set(log.counts)
    assert "kway_rows_kernel" not in log.counts and KERNEL not in log.counts
    assert log.counts["kway_anchor_rows_kernel"] == 3 + 1 and log.counts["segtopk_merge_kernel"] == 3      # 2 070 rows in chunks of 999
    with _lib.launch_log() as log:
        SW.kway_sweep(clf, lo, lo + 20, 3, 2, top=10)
    assert {"kway_rows_kernel", "topk_init_kernel", "topk_read_kernel"} | SELECT_KERNELS <= set(log.counts)
    assert log.counts["kway_rows_kernel"] == 2 and log.counts["topk_merge_kernel"] == 1 and KERNEL not in log.counts
    assert "kway_anchor_rows_kernel" not in log.counts


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_complete(tmp_path):
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
        json.dump({"temp_dir": temp, "resolution": R.FIXTURE_RES, "chrom_list": names, "min_distance": 0}, f)
    rng = np.random.default_rng(3)
    lo, hi = int(cr[2][0]), int(cr[2][1])
    away = np.asarray([v for v in range(1, 65) if not lo - 1 <= v <= hi])                 # the cluster of 25 keeps clear of the partner region
    clusters = [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s, pool in ((1, np.arange(1, 65)), (9, np.arange(1, 65)), (25, away))]
    ipath = os.path.join(tmp_path, "clusters.txt")
    with open(ipath, "w") as f:
        for ids in clusters:
            items = []
            for v in rng.permutation(ids):                               # unsorted on the line, positions anywhere inside their bins
                c, s = node2bin[int(v)].split(":")
                items.append("%s:%d" % (c, int(s) + R.FIXTURE_RES // 3))
            f.write("\t".join(items) + "\n\n")                           # an empty line behind each: line numbers 1, 3, 5
    bin2node = {v: key for key, v in node2bin.items()}
    clf = load_tiny("table")

    def run(free, *extra):
        out = os.path.join(tmp_path, "complete.tsv")
        PR.main(["complete", "-i", ipath, "--chrom", "2", "--free", str(free), "--top", "6", "-o", out, "--config", cpath, *extra])
        with np.load(os.path.join(tmp_path, "complete.npz")) as f:      # read now: the next run writes the same file
            z = {key: f[key] for key in f.files}
        assert set(z) == {"clusters", "rows", "added", "logit", "proba", "rank", "count"}
        assert np.array_equal(z["clusters"], CR.padded(clusters))
        lines = [line.rstrip("\n").split("\t") for line in open(out)]
        assert len(lines) == int(z["count"].sum())
        at = 0
        for a in range(3):                                               # grouped by cluster, best first
            for add, p in zip(z["added"][a, :z["count"][a]], z["proba"][a, :z["count"][a]]):
                assert int(lines[at][0]) == 2 * a + 1 and [bin2node[item] for item in lines[at][1:1 + free]] == add.tolist()
                assert np.float32(float(lines[at][1 + free])) == p
                at += 1
        return z

    def same(z, ref):
        return all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in KEYS)

    z = run(1)
    assert z["rows"].shape == (3, 6, 26) and z["count"][0] == z["count"][2] == 6 and 1 <= z["count"][1] <= 6
    assert same(z, SW.completion_sweep(clf, clusters, lo, hi, free=1, min_gap=1, top=6))         # min_gap = min_distance + 1
    w = run(2, "--start-bin", "2", "--end-bin", "14", "--width", "32", "--chunk-rows", "50")
    assert w["rows"].shape == (3, 6, 32)
    assert same(w, SW.completion_sweep(clf, clusters, lo + 2, lo + 14, free=2, min_gap=1, top=6, width=32))
    # --exclude-known drops the rows of all_<k>_counter.npy for the sizes present (2, 10 and 26 here; 10 has no file)
    np.save(os.path.join(temp, "all_2_counter.npy"), z["rows"][0, [0, 3], :2])
    np.save(os.path.join(temp, "all_26_counter.npy"), z["rows"][2, [1], :26])
    e = run(1, "--exclude-known")
    more = SW.completion_sweep(clf, clusters, lo, hi, free=1, min_gap=1, top=8)["rows"].cpu().numpy()
    assert np.array_equal(e["rows"][0], more[0][[1, 2, 4, 5, 6, 7]]) and np.array_equal(e["rows"][2], more[2][[0, 2, 3, 4, 5, 6]])
    assert np.array_equal(e["rows"][1], more[1, :6])
