"""Cluster decomposition on the MI355X (csrc/sweep_rows.hip's cluster_subset_rows_kernel and csrc/sweep_support.hip's subset_support_update_kernel, matcha_amd/sweep.py,
DESIGN.md 7.11): candidate rows and flags bit for bit against the itertools twin (tests/subsets_ref.py); the support planes bit for bit
against its integer restatement, whatever the cut and the order; the sweep against the reference's own logits per cluster (g16),
independent of how it is cut and of how the clusters are grouped; exclusion, errors and empty cases; the untouched sweeps; the CLI."""
import json
import math
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
from tests import subsets_ref as SR
from tests.helpers import GOLD, gold, logit_err
from tests.test_cpu_subsets import g16_case
from tests.test_hip_kway import SELECT_KERNELS, load_tiny
from tests.test_hip_long_rows import LONG, SHORT_ONLY

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
KERNEL = "cluster_subset_rows_kernel"
SUPPORT = "subset_support_update_kernel"
SEG_KERNELS = {"segtopk_keys_kernel", "segtopk_merge_kernel", "segtopk_commit_kernel"}
TENSORS = ("rows", "logit", "proba", "rank", "count", "chosen", "support_sum", "support_count", "support_mean")
DROP_ONLY = ("full_logit", "full_proba")


def got_np(pair):
    x, flag = pair
    assert x.dtype == torch.long and flag.dtype == torch.int32 and flag.shape == (x.shape[0],)
    return x.cpu().numpy(), flag.cpu().numpy() != 0


def ref_rows(table, m, comp, gap, L, granks):
    """The twin on a list of global ranks: (rows [n, L], invalid [n]); the choice of a rank from the twin's list, or, where C(S, m) is
    too large to list, from the Python unranking that tests/test_cpu_subsets.py holds against that list."""
    S = table.shape[1]
    cm = math.comb(S, m)
    listed = SR.choices(S, m) if cm <= 5000 else None
    rows, bad = np.zeros((len(granks), L), dtype=np.int64), np.ones(len(granks), dtype=bool)
    for i, g in enumerate(granks):
        if not 0 <= g < len(table) * cm:
            continue                                                     # out of range: a zero row with its flag set
        a, r = divmod(int(g), cm)
        choice = listed[r] if listed else SW._choice_unrank(r, S, m)
        row, ok, _ = SR.candidate(table[a], S, choice, comp, gap)
        rows[i, :len(row)] = row
        bad[i] = not ok
    return rows, bad


def mixed_table(rng, S, m):
    """Clusters with s_a = 0, 1, m, S - 1 and S in one table [A, S], ids 1 .. 3 S so that neighbours within a gap of 3 occur; one row
    that repeats an id."""
    pool = np.arange(1, 3 * S + 1)
    sizes = sorted({0, 1, min(m, S), S - 1, S})
    clusters = [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s in sizes]
    rep = sorted(int(v) for v in rng.choice(pool, size=S - 1, replace=False))
    clusters.append(sorted(rep + [rep[len(rep) // 2]]))
    return SR.padded(clusters, S)


# ---- rows and flags, exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8, 9, 32])
def test_rows_grid(S):
    rng = np.random.default_rng(200 + S)
    seen = set()
    for m, comp in ((1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (8, 0), (8, 1)):
        table = mixed_table(rng, S, m)
        A, cm = len(table), math.comb(S, m)
        dev_table = torch.from_numpy(table).cuda()
        if cm == 0:                                                      # m > S: no candidates, nothing launched
            with _lib.launch_log() as log:
                assert SW._subset_rows(dev_table, m, comp, 1, 0, None, None, 32, None, None)[0].shape == (0, 32)
            assert not log.counts
            continue
        total = A * cm
        if total <= 4000:
            granks, listed = np.arange(total), False
        else:                                                            # S = 32, m = 3 or 8: a rank list around the segments' ends
            edge = np.concatenate([[a * cm, a * cm + 1, (a + 1) * cm - 1] for a in range(A)])
            granks, listed = np.concatenate([edge, rng.integers(0, total, 2500)]), True
        for g in (1, 3):
            l_min = max(S - m, 1) if comp else m
            ref32, bad = ref_rows(table, m, comp, g, 32, granks)
            for L in sorted({l_min, 32}):
                ref = ref32[:, :L]
                assert not ref32[:, L:].any()
                with _lib.launch_log() as log:
                    if listed:
                        x, inv = got_np(SW._subset_rows(dev_table, m, comp, g, 0, None, torch.from_numpy(granks).cuda(), L, None, None))
                    else:
                        x, inv = got_np(SW._subset_rows(dev_table, m, comp, g, 0, None, None, L, None, None))
                assert x.shape == ref.shape and np.array_equal(x, ref) and np.array_equal(inv, bad), (S, m, comp, g, L)
                assert log.counts == {KERNEL: 1}                         # it, and only it
                seen.add((m, comp, g, L == 32))
            if g == 1 and (S - m >= 2 if comp else S >= m):
                assert bad.any() and not bad.all(), (S, m, comp, g)      # the short clusters are flagged, the long ones have valid rows
        if listed:                                                       # ... and ranges at both ends of the rank space
            for rank0, count in ((0, 65), (total - 4099, 4099), (3 * cm - 30, 63)):
                ref, bad = ref_rows(table, m, comp, 1, 32, np.arange(rank0, rank0 + count))
                x, inv = got_np(SW._subset_rows(dev_table, m, comp, 1, rank0, count, None, 32, None, None))
                assert np.array_equal(x, ref) and np.array_equal(inv, bad), (S, m, comp, rank0)
        # the same clusters as id lists of different lengths: the wrapper pads them
        lists = [SR.leading_ids(r) for r in table]
        if not listed:
            ref, bad = ref_rows(table, m, comp, 1, 32, granks)
            x2, inv2 = got_np(SW.subset_rows(lists, m, comp, 1, width=32))
            assert np.array_equal(x2, ref) and np.array_equal(inv2, bad)
    assert ((2, 0, 3, True) in seen) and ((1, 1, 1, False) in seen) and ((8, 0, 1, True) in seen) == (S >= 8)


def test_rows_ranges_counts_and_rank_lists():
    """60 clusters of 0 .. 9 ids, three of nine positions: 5 040 ranks.  Ranges that begin and end inside a cluster's segment, counts
    around a wavefront and over many blocks, a rank list with out-of-range and repeated entries, reused buffers."""
    m, comp, g, S, L = 3, 0, 1, 9, 5
    rng = np.random.default_rng(8)
    clusters = [sorted(int(v) for v in rng.choice(np.arange(1, 60), size=int(s), replace=False)) for s in rng.integers(0, S + 1, size=60)]
    clusters[3], clusters[17] = list(range(2, 2 + S)), []
    table = SR.padded(clusters, S)
    ref, bad = SR.table(table, S, m, comp, g, L)
    cm = 84
    assert len(ref) == 60 * cm == SW.subset_count(60, S, m)
    dev_table = torch.from_numpy(table).cuda()
    for comp2 in (0, 1):
        L2 = L if comp2 == 0 else 7
        ref2, bad2 = (ref, bad) if comp2 == 0 else SR.table(table, S, m, 1, g, L2)
        for count in (1, 63, 64, 65, 4099):
            for rank0 in (0, 3 * cm + 41, len(ref2) - count):
                x, inv = got_np(SW.subset_rows(dev_table, m, comp2, g, rank0=rank0, count=count, width=L2))
                assert np.array_equal(x, ref2[rank0:rank0 + count]) and np.array_equal(inv, bad2[rank0:rank0 + count]), (comp2, rank0, count)
    with pytest.raises(IndexError):
        SW.subset_rows(dev_table, m, comp, g, rank0=len(ref) - 1, count=2, width=L)
    total = len(ref)
    ranks = np.concatenate([rng.permutation(total)[:700], rng.integers(0, total, 300), [-1, total, 1 << 62, -(1 << 40), 0, 0, total - 1]])
    rng.shuffle(ranks)
    with _lib.launch_log() as log:
        x, inv = got_np(SW.subset_rows(dev_table, m, comp, g, ranks=torch.from_numpy(ranks).cuda(), width=L))
    assert log.counts == {KERNEL: 1}                                     # the same kernel as the range form
    ok = (ranks >= 0) & (ranks < total)
    assert np.array_equal(x[ok], ref[ranks[ok]]) and np.array_equal(inv[ok], bad[ranks[ok]])
    assert not x[~ok].any() and inv[~ok].all() and (~ok).sum() == 4      # out of range: a zero row with its flag set
    # no clusters: every listed rank is out of range, and the range form is empty
    x, inv = got_np(SW.subset_rows(np.zeros((0, 3), dtype=np.int64), 2, ranks=torch.tensor([0, 1], device="cuda")))
    assert not x.any() and inv.all()
    with _lib.launch_log() as log:
        assert SW.subset_rows(np.zeros((0, 3), dtype=np.int64), 2, device="cuda")[0].shape[0] == 0
    assert not log.counts
    buf = torch.full((100 * L,), -7, dtype=torch.long, device="cuda")
    fbuf = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    x, flag = SW.subset_rows(dev_table, m, comp, g, rank0=130, count=40, width=L, out=buf, flag_out=fbuf)
    assert x.data_ptr() == buf.data_ptr() and flag.data_ptr() == fbuf.data_ptr()
    assert np.array_equal(x.cpu().numpy(), ref[130:170]) and np.array_equal(flag.cpu().numpy() != 0, bad[130:170])
    assert bool((buf[40 * L:] == -7).all()) and bool((fbuf[40:] == -7).all())


def test_c_contract_reads_the_leading_run_and_flags_a_descending_row():
    """Tables handed straight to the C entry point, as they stand: ids behind the first zero are ignored; every candidate of a row that
    descends somewhere is flagged and keeps its ids in position order; the wrapper sorts the same rows first."""
    S, L = 6, 6
    raw = [[40, 7, 9, 0, 0, 0], [3, 9, 0, 50, 2, 0], [0, 8, 9, 0, 0, 0], [7, 7, 12, 30, 0, 0], [2, 6, 10, 11, 25, 4], [1, 3, 5, 7, 9, 11]]
    table = torch.tensor(raw, dtype=torch.long, device="cuda")
    for m, comp, g in ((2, 0, 1), (1, 1, 1), (2, 1, 2), (3, 0, 2)):
        ref, bad = SR.table(raw, S, m, comp, g, L)
        x, inv = got_np(SW._subset_rows(table, m, comp, g, 0, None, None, L, None, None))
        assert np.array_equal(x, ref) and np.array_equal(inv, bad), (m, comp, g)
        cm = math.comb(S, m)
        assert bad[:cm].all() and bad[2 * cm:3 * cm].all() and bad[4 * cm:5 * cm].all()   # a descent, no leading id, a descent at the last id
        assert not ref[2 * cm:3 * cm].any()                                            # no id: every choice reaches past the ids
        assert not bad[5 * cm:].all()
    ref, bad = SR.table(raw, S, 2, 0, 1, L)
    assert np.array_equal(ref[0, :3], [40, 7, 0]) and np.array_equal(ref[1, :3], [40, 9, 0]) and not ref[2].any()      # position 3 holds no id
    assert np.array_equal(ref[15, :3], [3, 9, 0]) and not bad[15] and bad[16:30].all()       # [3, 9]: what stands behind the zero is ignored
    assert bad[45] and np.array_equal(ref[45, :2], [7, 7]) and not bad[46]                   # a repeated id; (7, 12) is fine
    xs, invs = got_np(SW.subset_rows(raw, 2, 0, 1, width=L))                                 # the wrapper: every row sorted, zeros last
    srt = SR.padded([sorted(v for v in r if v) for r in raw], S)
    ref_s, bad_s = SR.table(srt, S, 2, 0, 1, L)
    assert np.array_equal(xs, ref_s) and np.array_equal(invs, bad_s) and not bad_s[:15].all() and not bad_s[60:75].any()


# ---- the support planes ------------------------------------------------------------------------------------------------------------------
def support_np(sup):
    z = sup.read()
    return z["sum"].cpu().numpy(), z["count"].cpu().numpy(), z["counters"].cpu().tolist()


def awkward_values(rng, n):
    """float32 values in [0, 1] with rejected ones (NaN, negative, too large, +inf), -0.0 and exact ends, and a skip mask."""
    v = rng.random(n).astype(np.float32)
    at = rng.permutation(n)[:12]
    v[at] = [np.nan, -1e-3, 1.0000001, np.inf, -0.0, 0.0, 1.0, 1e-12, -np.inf, 2.0, 0.5, np.nan]
    skip = rng.random(n) < 0.15
    skip[at[:2]] = False
    skip[at[2]] = True                                                   # a skipped row is not rejected, whatever its value
    return v, skip


@pytest.mark.parametrize("A,S,m", [(60, 9, 3), (5000, 3, 2), (12, 32, 2), (40, 8, 8), (3, 32, 1)])
def test_support_planes_bitwise(A, S, m):
    """(60, 9, 3): a block's run of 2 048 ranks spans 25 clusters, inside the LDS tile of 1 024 / 9 = 113; (5 000, 3, 2): it spans 683,
    the tile holds 341 and the rest goes to global atomics; (12, 32, 2): 5 clusters of 32 cells; (40, 8, 8): one choice per cluster."""
    cm = math.comb(S, m)
    n = A * cm
    rng = np.random.default_rng(A + S + m)
    v, skip = awkward_values(rng, n)
    want_sum, want_cnt, want_counters = SR.support(A, S, m, v, skip, 0)
    vd, sd = torch.from_numpy(v).cuda(), torch.from_numpy(skip).cuda()
    first = None
    for chunk in (n, 37 if n <= 6000 else 1501, 4099):
        sup = SW.SubsetSupport(A, S, m, device="cuda")
        with _lib.launch_log() as log:
            for g0 in range(0, n, chunk):
                sup.update(vd[g0:g0 + chunk], g0, sd[g0:g0 + chunk])
        assert log.counts == {SUPPORT: -(-n // chunk)}                   # its own kernel only
        got = support_np(sup)
        assert np.array_equal(got[0], want_sum) and np.array_equal(got[1], want_cnt) and got[2] == want_counters, (A, S, m, chunk)
        if first is None:
            first = sup.state.clone()
        else:
            assert torch.equal(sup.state, first)                         # the whole state, header and padding included
    # a shuffled order of the same chunks, and a bool-free call (no skip) on top of an int32 one
    sup = SW.SubsetSupport(A, S, m, device="cuda")
    starts = list(range(0, n, 4099))
    for g0 in rng.permutation(starts):
        sup.update(vd[g0:g0 + 4099], int(g0), sd[g0:g0 + 4099].to(torch.int32))
    assert torch.equal(sup.state, first)
    # the exact identities
    live = ~skip & (v >= 0) & (v <= 1)
    assert want_counters == [int(live.sum()), int((~skip & ~live).sum())] and want_counters[1] >= 4
    got_sum, got_cnt, _ = support_np(sup)
    q = np.asarray([SR.quantum(x) if ok else 0 for x, ok in zip(v, live)], dtype=np.int64)
    assert np.array_equal(got_cnt.sum(axis=1), m * live.reshape(A, cm).sum(axis=1))
    assert np.array_equal(got_sum.sum(axis=1), m * q.reshape(A, cm).sum(axis=1))
    # without a skip mask every row is accepted or rejected; a larger vmax accepts more
    sup = SW.SubsetSupport(A, S, m, vmax=2.0, device="cuda")
    sup.update(vd, 0)
    w = SR.support(A, S, m, v, None, 0, vmax=2.0)
    got = support_np(sup)
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2] and got[2][0] + got[2][1] == n


def test_support_refusals_on_the_device():
    sup = SW.SubsetSupport(4, 9, 3, device="cuda")
    v = torch.zeros(10, device="cuda")
    with _lib.launch_log() as log:
        with pytest.raises(_lib.MatchaHipError, match="outside"):
            sup.update(v, 4 * 84 - 9)
        with pytest.raises(ValueError):
            sup.update(v.double(), 0)
        with pytest.raises(ValueError):
            sup.update(v, 0, torch.zeros(9, device="cuda"))
        sup.update(v[:0], 0)                                             # nothing to do: nothing launched
        for bad in ((0, 9, 3), (4, 1, 3), (4, 33, 3), (4, 9, 0), (4, 9, 9)):
            with pytest.raises(ValueError):
                SW.SubsetSupport(*bad, device="cuda")
        with pytest.raises(ValueError):
            SW.SubsetSupport(4, 9, 3, vmax=0.0, device="cuda")
    assert not log.counts
    total, cnt, counters = support_np(sup)
    assert not total.any() and not cnt.any() and counters == [0, 0]


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_decomposition_sweep_against_reference_logits(mode):
    g = gold("g16_subsets_tiny.npz")
    clf = load_tiny(mode)
    for i in range(len(SR.G16_CASES)):
        clusters, m, comp, gap, W = g16_case(g, i)
        rows, valid, off = g[f"rows_c{i}"].astype(np.int64), g[f"valid_c{i}"], g[f"offsets_c{i}"]
        ref, ksel, ref_sup = g[f"logit_{mode}_c{i}"].astype(np.float64), g[f"ksel_{mode}_c{i}"], g[f"support_{mode}_c{i}"]
        A, top = len(clusters), 8                                        # the largest K_a there can be; cut per cluster below
        with _lib.launch_log() as log:
            out = SW.decomposition_sweep(clf, clusters, m, mode="drop" if comp else "keep", min_gap=gap, top=top, width=W)
        ran = {name for name, c in log.counts.items() if c > 0}
        if W > 8:
            assert LONG <= ran and not (ran & SHORT_ONLY), sorted(ran)   # the long plan and attention
        else:
            assert ran & SHORT_ONLY and not (ran & LONG), sorted(ran)    # the L <= 8 kernels
        assert not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)                 # no training kernel
        n_sizes = len(set(len(c) for c in clusters))
        assert log.counts[SUPPORT] == n_sizes == log.counts["segtopk_merge_kernel"] and "kway_complete_rows_kernel" not in ran
        assert log.counts[KERNEL] == n_sizes * (2 if m == 1 else 3)       # the sweep, the winners' rows and (m >= 2) their chosen ids
        assert out["n_candidates"] == len(rows) and out["n_invalid"] == int((~valid).sum()) and out["n_excluded"] == 0
        assert out["rows"].shape == (A, top, W) and out["chosen"].shape == (A, top, m) and out["logit"].shape == (A, top)
        for a in range(A):
            lo, s = int(off[a]), len(clusters[a])
            ok = np.flatnonzero(valid[lo:int(off[a + 1])])
            count = int(out["count"][a])
            assert count == min(top, len(ok))
            K = int(ksel[a])
            rank = out["rank"][a, :K].cpu().numpy()
            assert np.isin(rank, ok).all() and len(set(rank.tolist())) == K
            logit = out["logit"][a, :K].cpu().numpy()
            e = logit_err(logit, ref[lo + rank])
            print(f"{mode} case {i} cluster {a}: logit_err {e:.2e}")
            assert e <= TOL, (mode, i, a, e)
            assert set(rank.tolist()) == set(ok[np.argsort(-ref[lo + ok])[:K]].tolist()), (mode, i, a)         # the reference's top K_a
            assert np.allclose(np.sort(logit)[::-1], logit)                                                    # best first
            kept_rows = out["rows"][a, :count].cpu().numpy()
            assert np.array_equal(kept_rows, rows[lo + out["rank"][a, :count].cpu().numpy()])
            for row, ch, r in zip(kept_rows.tolist(), out["chosen"][a, :count].tolist(), out["rank"][a, :count].tolist()):
                ids = [v for v in row if v]
                assert (sorted(ids + ch) == clusters[a] and not set(ids) & set(ch)) if comp else ids == ch
                assert ch == [clusters[a][p] for p in SR.choices(s, m)[r]]
                assert SW.subset_unrank(r, clusters[a], m, comp, gap) == (tuple(ids), True)
            assert bool((out["rank"][a, count:] == -1).all()) and not out["rows"][a, count:].any() and not out["chosen"][a, count:].any()
            assert not out["logit"][a, count:].any() and not out["proba"][a, count:].any()
            # the per-locus support against the reference's float64 sums
            got = out["support_sum"][a, :s].cpu().numpy()
            rel = float(np.abs(got - ref_sup[a, :s]).max() / np.abs(ref_sup[a, :s]).max())
            print(f"{mode} case {i} cluster {a}: support_sum rel {rel:.2e}")
            assert rel <= TOL, (mode, i, a, rel)
            want_cnt = np.zeros(s, dtype=np.int64)
            for r in ok:
                want_cnt[list(SR.choices(s, m)[r])] += 1
            assert np.array_equal(out["support_count"][a, :s].cpu().numpy(), want_cnt)
            assert not out["support_sum"][a, s:].any() and not out["support_count"][a, s:].any()
        kept = out["rank"] >= 0
        assert torch.equal(out["proba"][kept], torch.sigmoid(out["logit"][kept]))
        hit = out["support_count"] > 0
        assert torch.equal(out["support_mean"][hit], (out["support_sum"][hit] / out["support_count"][hit]).float()) and not out["support_mean"][~hit].any()
        if comp:
            e = logit_err(out["full_logit"].cpu().numpy(), g[f"full_{mode}_c{i}"].astype(np.float64))
            print(f"{mode} case {i}: full_logit logit_err {e:.2e}")
            assert e <= TOL and torch.equal(out["full_proba"], torch.sigmoid(out["full_logit"]))
        else:
            assert "full_logit" not in out and "full_proba" not in out
        for chunk_rows in (37, 4099):                                    # the cut is not part of the result
            again = SW.decomposition_sweep(clf, clusters, m, mode="drop" if comp else "keep", min_gap=gap, top=top, width=W, chunk_rows=chunk_rows)
            assert all(torch.equal(again[key], out[key]) for key in TENSORS + (DROP_ONLY if comp else ())), (mode, i, chunk_rows)


# ---- the sweep's behaviour -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d64():
    """The d = 64 table model of tests/test_hip_kway.py on hg38 at 1 Mb."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    cr = np.asarray(synth.chrom_range(num))
    c = num.index(48)
    clf, _ = hip_model(num, 64, "table", 12)
    return dict(clf=clf.eval(), lo=int(cr[c][0]), hi=int(cr[c][1]), N=int(np.sum(num)), chr1=(int(cr[0][0]), int(cr[0][1])))


def d64_clusters(d64, rng, sizes):
    """Clusters across chromosome 1 and the 48-bin chromosome."""
    pool = np.concatenate([np.arange(*d64["chr1"]), np.arange(d64["lo"], d64["hi"])])
    return [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s in sizes]


def same(a, b, keys):
    return all(torch.equal(a[key], b[key]) for key in keys) and all(a[key] == b[key] for key in ("n_candidates", "n_invalid", "n_excluded"))


def test_sweep_does_not_depend_on_the_cut_or_the_grouping_d64(d64):
    clf = d64["clf"]
    rng = np.random.default_rng(22)
    ragged = d64_clusters(d64, rng, [9, 25, 12, 9, 2, 20, 12, 17, 3, 1])
    for mode, m, width, long_rows in (("keep", 3, None, False), ("keep", 2, 8, False), ("drop", 1, None, True), ("drop", 2, 32, True)):
        keys = TENSORS + (DROP_ONLY if mode == "drop" else ())
        first = None
        for chunk_rows in (None, 37, 4099):
            with _lib.launch_log() as log:
                out = SW.decomposition_sweep(clf, ragged, m, mode=mode, min_gap=2, top=30, width=width, chunk_rows=chunk_rows)
            ran = {name for name, c in log.counts.items() if c > 0}
            assert (LONG <= ran and not (ran & SHORT_ONLY)) if long_rows else (ran & SHORT_ONLY and not (ran & LONG)), sorted(ran)
            assert not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)
            if first is None:
                first = out
                assert out["rows"].shape[2] == (width or (25 if mode == "drop" else m)) and out["n_invalid"] > 0
                small = [a for a, c in enumerate(ragged) if (len(c) - m < 2 if mode == "drop" else len(c) < m)]
                assert small and not out["count"][small].any() and bool((out["count"][[0, 1, 2]] > 0).all())
            else:
                assert same(out, first, keys), (mode, m, width, chunk_rows)
        # a ragged table equals the concatenation of per-size runs
        W = first["rows"].shape[2]
        K = first["rows"].shape[1]
        for s in sorted(set(len(c) for c in ragged)):
            idx = [a for a, c in enumerate(ragged) if len(c) == s]
            alone = SW.decomposition_sweep(clf, [ragged[a] for a in idx], m, mode=mode, min_gap=2, top=30, width=W)
            Ks = alone["rows"].shape[1]
            for key in keys:
                part = first[key][idx]
                if key in ("rows", "logit", "proba", "rank", "chosen"):
                    assert torch.equal(part[:, :Ks], alone[key]), (mode, m, s, key)
                    assert not part[:, Ks:].any() if key != "rank" else bool((part[:, Ks:] == -1).all())
                elif key.startswith("support"):
                    assert torch.equal(part[:, :alone[key].shape[1]], alone[key]) and not part[:, alone[key].shape[1]:].any(), (mode, m, s, key)
                else:
                    assert torch.equal(part, alone[key]), (mode, m, s, key)
        # the kept logits are model(x)'s on the kept rows, on the same route
        with torch.no_grad(), _lib.option("disable_small_batch"):
            direct = clf(first["rows"].view(-1, W)).view(first["logit"].shape)
        kept = first["rank"] >= 0
        assert float((direct[kept] - first["logit"][kept]).abs().max()) <= 1e-6     # what two batchings of one forward may differ by
        # without the support planes: the same selection, no support kernel
        with _lib.launch_log() as log:
            bare = SW.decomposition_sweep(clf, ragged, m, mode=mode, min_gap=2, top=30, width=width, support=False, task_mode="regress")
        assert SUPPORT not in log.counts and "support_sum" not in bare and torch.equal(bare["rank"], first["rank"])
        assert torch.equal(bare["proba"][kept], torch.nn.functional.softplus(bare["logit"][kept]))


def test_exclude_counts_and_kept_ranks(d64):
    clf = d64["clf"]
    m, gap, top = 2, 2, 496                                              # C(32, 2): every valid candidate is kept
    clusters = d64_clusters(d64, np.random.default_rng(7), [32, 25, 32, 9])
    by_cluster = [SR.table([c], len(c), m, 1, gap, 32) for c in clusters]
    ref, bad = np.concatenate([r for r, _ in by_cluster]), np.concatenate([b for _, b in by_cluster])
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in by_cluster])])
    assert bad.any() and not bad.all()
    known = np.concatenate([np.flatnonzero(~bad)[::5], np.flatnonzero(bad)[::3]])      # some valid and some invalid candidates
    hset = HyperedgeSet(torch.from_numpy(ref[known]).cuda())
    assert hset.L == 32
    out = SW.decomposition_sweep(clf, clusters, m, mode="drop", min_gap=gap, top=top, width=32, exclude=hset, chunk_rows=50)
    assert out["n_excluded"] == len(np.flatnonzero(~bad)[::5]) and out["n_invalid"] == int(bad.sum()) and out["n_candidates"] == len(ref)
    left = ~bad
    left[known] = False
    for a in range(len(clusters)):
        want = np.flatnonzero(left[off[a]:off[a + 1]])
        assert int(out["count"][a]) == len(want)
        assert set(out["rank"][a, :len(want)].tolist()) == set(want.tolist()) and bool((out["rank"][a, len(want):] == -1).all())
        cnt = np.zeros(len(clusters[a]), dtype=np.int64)
        for r in want:
            cnt[list(SR.choices(len(clusters[a]), m)[r])] += 1
        assert np.array_equal(out["support_count"][a, :len(cnt)].cpu().numpy(), cnt)      # excluded rows do not count
    everything = SW.decomposition_sweep(clf, clusters, m, mode="drop", min_gap=gap, top=top, width=32)
    assert everything["n_excluded"] == 0 and int(everything["count"].sum()) == int((~bad).sum())


def test_errors_and_empty_cases(d64):
    clf = d64["clf"]
    clusters = d64_clusters(d64, np.random.default_rng(6), [12, 3])
    clf._runtime()                                                       # (packing the model's parameters is not the sweep's doing)
    with _lib.launch_log() as log:
        for kw in (dict(m=1), dict(m=9), dict(m=3, width=2), dict(m=3, width=9), dict(m=3, mode="other"), dict(m=3, top=0), dict(m=3, min_gap=0),
                   dict(m=3, task_mode="other"), dict(m=3, task_mode="regress"), dict(m=0, mode="drop"), dict(m=9, mode="drop"),
                   dict(m=1, mode="drop", width=11), dict(m=1, mode="drop", width=33), dict(m=1, mode="drop", width=32, chunk_rows=1 << 27),
                   dict(m=3, chunk_rows=0)):
            with pytest.raises(ValueError):
                SW.decomposition_sweep(clf, clusters, **kw)
        with pytest.raises(ValueError):
            SW.decomposition_sweep(clf, [list(range(1, 34))], 2)         # a cluster of 33 ids
        # no clusters, clusters all too small: nothing is launched
        for tab, m, mode in (([], 3, "keep"), ([], 1, "drop"), ([[5, 9], [7]], 3, "keep"), ([[5, 9, 11], [7, 8], []], 2, "drop")):
            empty = SW.decomposition_sweep(clf, tab, m, mode=mode)
            W = m if mode == "keep" else max([len(c) for c in tab] + [2])
            assert empty["n_candidates"] == 0 and empty["rows"].shape == (len(tab), 0, W) and empty["chosen"].shape == (len(tab), 0, m)
            assert all(empty[key].shape == (len(tab), 0) and empty[key].is_cuda for key in ("logit", "proba", "rank"))
            assert empty["count"].shape == (len(tab),) and not empty["count"].any() and not empty["support_count"].any()
            assert ("full_logit" in empty) == (mode == "drop")
    assert not log.counts
    with pytest.raises(IndexError):
        SW.decomposition_sweep(clf, [clusters[0], [3, 9, d64["N"] + 5]], 2)     # a cluster id beyond the model's table: once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    a, b = SW.decomposition_sweep(clf, clusters, 2, top=5), SW.decomposition_sweep(clf, clusters, 2, top=5)
    assert same(a, b, TENSORS) and a["rows"].shape == (2, 5, 2) and a["count"].tolist() == [5, 3]
    full = SW.decomposition_sweep(clf, [list(range(40, 72))], 1, mode="drop", top=3)      # 32 ids: allowed here
    assert full["rows"].shape == (1, 3, 32) and int(full["count"][0]) == 3 and bool((full["rows"][0, :, 30] > 0).all()) and not full["rows"][0, :, 31].any()


def test_the_other_sweeps_launch_what_they_launched(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    new = {KERNEL, SUPPORT, "subset_support_init_kernel", "subset_support_read_kernel"}
    with _lib.launch_log() as log:
        SW.anchored_sweep(clf, np.asarray([d64["chr1"][0], d64["chr1"][0] + 9]), lo, hi, 3, 3, top=10, chunk_rows=999)
    assert {"kway_anchor_rows_kernel", "segtopk_init_kernel", "segtopk_read_kernel"} | SEG_KERNELS <= set(log.counts)
    assert "kway_rows_kernel" not in log.counts and not new & set(log.counts)
    assert log.counts["kway_anchor_rows_kernel"] == 3 + 1 and log.counts["segtopk_merge_kernel"] == 3      # 2 070 rows in chunks of 999
    with _lib.launch_log() as log:
        SW.kway_sweep(clf, lo, lo + 20, 3, 2, top=10)
    assert {"kway_rows_kernel", "topk_init_kernel", "topk_read_kernel"} | SELECT_KERNELS <= set(log.counts)
    assert log.counts["kway_rows_kernel"] == 2 and log.counts["topk_merge_kernel"] == 1 and not new & set(log.counts)
    assert "kway_anchor_rows_kernel" not in log.counts
    with _lib.launch_log() as log:
        SW.completion_sweep(clf, [[d64["chr1"][0] + 1, d64["chr1"][0] + 7], [d64["chr1"][0] + 3]], lo, hi, free=1, top=10, chunk_rows=50)
    assert log.counts["kway_complete_rows_kernel"] == 2 + 2 and log.counts["segtopk_merge_kernel"] == 2    # 96 rows in chunks of 50
    assert "kway_anchor_rows_kernel" not in log.counts and "kway_rows_kernel" not in log.counts and not new & set(log.counts)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_decompose(tmp_path):
    num = R.FIXTURE_LAYOUTS["tiny"]
    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    node2bin, names = R.fixture_node2bin(num)
    np.save(os.path.join(temp, "node2bin.npy"), node2bin, allow_pickle=True)
    np.save(os.path.join(temp, "chrom_range.npy"), np.asarray(synth.chrom_range(num)))
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": R.FIXTURE_RES, "chrom_list": names, "min_distance": 0}, f)
    rng = np.random.default_rng(3)
    clusters = [sorted(int(v) for v in rng.choice(np.arange(1, 65), size=s, replace=False)) for s in (2, 9, 25)]
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

    def run(size, *extra):
        out = os.path.join(tmp_path, "decompose.tsv")
        PR.main(["decompose", "-i", ipath, "--size", str(size), "--top", "6", "-o", out, "--config", cpath, *extra])
        with np.load(os.path.join(tmp_path, "decompose.npz")) as f:     # read now: the next run writes the same file
            z = {key: f[key] for key in f.files}
        drop = "--drop" in extra
        assert set(z) == {"clusters", *TENSORS} | (set(DROP_ONLY) if drop else set())
        assert np.array_equal(z["clusters"], SR.padded(clusters))
        lines = [line.rstrip("\n").split("\t") for line in open(out)]
        assert len(lines) == int(z["count"].sum())
        at = 0
        for a in range(3):                                               # grouped by cluster, best first
            for ch, p in zip(z["chosen"][a, :z["count"][a]], z["proba"][a, :z["count"][a]]):
                assert int(lines[at][0]) == 2 * a + 1 and [bin2node[item] for item in lines[at][1:1 + size]] == ch.tolist()
                assert np.float32(float(lines[at][1 + size])) == p and len(lines[at]) == 2 + size + drop
                if drop:
                    assert abs(float(lines[at][2 + size]) - (float(p) - float(z["full_proba"][a]))) < 1e-12
                at += 1
        sup = [line.rstrip("\n").split("\t") for line in open(os.path.join(tmp_path, "decompose_support.tsv"))]
        assert len(sup) == 2 + 9 + 25
        at = 0
        for a in range(3):                                               # one line per cluster locus, in the cluster's order
            for j, v in enumerate(clusters[a]):
                assert int(sup[at][0]) == 2 * a + 1 and bin2node[sup[at][1]] == v
                assert np.float32(float(sup[at][2])) == z["support_mean"][a, j] and int(sup[at][3]) == z["support_count"][a, j]
                at += 1
        return z

    def agrees(z, ref, keys):
        return all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in keys)

    z = run(2)
    assert z["rows"].shape == (3, 6, 2) and z["count"].tolist() == [1, 6, 6]
    assert agrees(z, SW.decomposition_sweep(clf, clusters, 2, top=6), TENSORS)                       # min_gap = min_distance + 1
    w = run(3, "--width", "8", "--chunk-rows", "50", "--min-gap", "2")
    assert w["rows"].shape == (3, 6, 8) and w["count"][0] == 0
    assert agrees(w, SW.decomposition_sweep(clf, clusters, 3, min_gap=2, top=6, width=8), TENSORS)
    d = run(1, "--drop")
    assert d["rows"].shape == (3, 6, 25) and d["count"].tolist() == [0, 6, 6] and d["full_proba"][0] == 0 and d["full_proba"][1] > 0
    assert agrees(d, SW.decomposition_sweep(clf, clusters, 1, mode="drop", top=6), TENSORS + DROP_ONLY)
    # --exclude-known drops the rows of all_<k>_counter.npy for the candidate sizes present (8 and 24 here; 8 has no file)
    np.save(os.path.join(temp, "all_24_counter.npy"), d["rows"][2, [1], :24])
    e = run(1, "--drop", "--exclude-known")
    more = SW.decomposition_sweep(clf, clusters, 1, mode="drop", top=7)["rows"].cpu().numpy()
    assert np.array_equal(e["rows"][2], more[2][[0, 2, 3, 4, 5, 6]]) and np.array_equal(e["rows"][1], more[1, :6])
    # a bad line fails with its number before anything is scored
    with open(ipath, "a") as f:
        f.write("%s\n" % node2bin[5])
    with pytest.raises(ValueError, match=r"line 7 has 1 distinct bins"):
        PR.main(["decompose", "-i", ipath, "--size", "2", "--top", "6", "-o", os.path.join(tmp_path, "x.tsv"), "--config", cpath])
    assert not os.path.exists(os.path.join(tmp_path, "x.tsv"))
