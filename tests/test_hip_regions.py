"""The multi-region sweep on the MI355X (csrc/sweep_rows.hip, matcha_amd/sweep.py): candidate rows and their flags bit for
bit against region_unrank and itertools and, beyond 2^61, against Python integers; region_sweep against the reference's own logits
(g18), per leading candidate against the anchored sweep, and against one batch of the d = 64 model with parts on three chromosomes;
region_map against the numpy twin of the pair map; the CLI."""
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
from tests import regions_ref as RR
from tests.helpers import GOLD, gold
from tests.pairmap_ref import SCALE, pairmap_ref
from tests.test_cpu_regions import GRID, TINY

pytestmark = pytest.mark.gpu

TOL = 1e-4                       # the device forward against the reference's CPU logits (tests/test_hip_kway.py)
PLANES = ("sum", "count", "count_ge", "max")
KERNEL = "kway_region_rows_kernel"
_CACHE = {}


def brute(parts, gap, width=None):
    """(rows, invalid) by itertools, computed once per case and shared."""
    key = (tuple(parts), gap, width)
    if key not in _CACHE:
        rows, valid = RR.candidates(parts, gap, width)
        rows.setflags(write=False)
        _CACHE[key] = (rows, ~valid)
    return _CACHE[key]


def got_np(pair):
    x, flag = pair
    assert x.dtype == torch.long and flag.dtype == torch.int32 and flag.shape == (x.shape[0],)
    f = flag.cpu().numpy()
    assert ((f == 0) | (f == 1)).all()
    return x.cpu().numpy(), f != 0


def load_tiny(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    return torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False)


# ---- rows, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_region_rows_grid_against_unrank(wide):
    for parts, gap in GRID:
        k = sum(m for _, _, m in parts)
        width = 8 if wide else k
        ref, bad = brute(parts, gap, width)
        with _lib.launch_log() as log:
            x, inv = got_np(SW.region_rows(parts, gap, width=width))
        assert x.shape == ref.shape and np.array_equal(x, ref) and np.array_equal(inv, bad), (parts, gap)
        assert (set(log.counts) == {KERNEL}) if len(ref) else not log.counts      # it, and only it; nothing for an empty sweep
        step = 1 if len(ref) <= 3000 else 7
        for r in range(0, len(ref), step):                               # the Python decoder says the same, rank by rank
            row, ok = SW.region_unrank(r, parts, gap)
            assert tuple(x[r, :k]) == row and bool(inv[r]) == (not ok), (parts, gap, r)
        if len(parts) == 1 and len(ref):                                 # one part: kway_rows' rows, bit for bit
            lo, hi, m = parts[0]
            assert torch.equal(SW.region_rows(parts, gap, width=width)[0], SW.kway_rows(lo, hi - lo, m, gap, width=width)) and not inv.any()


def test_region_rows_ranges_inside_and_across_leading_segments():
    """Counts around a wave, over a block and over several blocks; from rank 0, from inside a segment of the leading part (its T / C_0
    consecutive ranks) and up to the last rank."""
    cases = [([(1 + 4 * p, 4 + 4 * p, 1) for p in range(8)], 1), ([(1 + 4 * p, 4 + 4 * p, 1) for p in range(8)], 3),
             ([(1, 13, 2), (13, 21, 1), (21, 33, 2)], 2)]
    for parts, gap in cases:
        ref, bad = brute(parts, gap, 8)
        T = len(ref)
        seg = T // SW.region_count(parts[:1] + [(10000, 10001, 1)], gap)  # T / C_0 (a second part makes k >= 2 for the count)
        assert T > 4099 + seg and (gap == 1 or (bad.any() and not bad.all()))
        for count in (1, 63, 64, 65, 4099):
            for rank0 in (0, min(seg + seg // 3, T - count - 1), T - count):      # the middle one begins inside a leading segment
                x, inv = got_np(SW.region_rows(parts, gap, rank0=rank0, count=count, width=8))
                assert np.array_equal(x, ref[rank0:rank0 + count]) and np.array_equal(inv, bad[rank0:rank0 + count]), (parts, gap, rank0, count)
        with pytest.raises(IndexError):
            SW.region_rows(parts, gap, rank0=T - 1, count=2)


def test_region_rows_list_form_and_reused_buffers():
    parts, gap = [(1, 9, 2), (9, 15, 1), (15, 23, 2)], 3
    ref, bad = brute(parts, gap, 6)
    total = len(ref)
    rng = np.random.default_rng(5)
    ranks = np.concatenate([rng.permutation(total), rng.integers(0, total, 300), [-1, total, 1 << 62, -(1 << 40), 0, total - 1]])
    rng.shuffle(ranks)
    with _lib.launch_log() as log:
        x, inv = got_np(SW.region_rows(parts, gap, ranks=torch.from_numpy(ranks).cuda(), width=6))
    assert log.counts == {KERNEL: 1}                                     # the same kernel as the range form
    ok = (ranks >= 0) & (ranks < total)
    assert np.array_equal(x[ok], ref[ranks[ok]]) and np.array_equal(inv[ok], bad[ranks[ok]])
    assert not x[~ok].any() and inv[~ok].all() and (~ok).sum() == 4      # out of range: a zero row with its flag set
    # a sweep without candidates: every listed rank is out of range
    empty = [(1, 7, 3), (40, 56, 2)]
    x, inv = got_np(SW.region_rows(empty, 4, ranks=torch.tensor([0, 1], device="cuda")))
    assert not x.any() and inv.all() and SW.region_rows(empty, 4, device="cuda")[0].shape == (0, 5)
    # ``out`` and ``flag_out`` reuse the caller's buffers and leave the memory behind ``count`` alone
    buf = torch.full((100 * 6,), -7, dtype=torch.long, device="cuda")
    fbuf = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    x, flag = SW.region_rows(parts, gap, rank0=10, count=40, width=6, out=buf, flag_out=fbuf)
    assert x.data_ptr() == buf.data_ptr() and flag.data_ptr() == fbuf.data_ptr()
    assert np.array_equal(x.cpu().numpy(), ref[10:50]) and np.array_equal(flag.cpu().numpy() != 0, bad[10:50])
    assert bool((buf[240:] == -7).all()) and bool((fbuf[40:] == -7).all())


def test_region_rows_large_ranks_against_python_integers():
    def check(parts, gap, ranks, width=None):
        k = sum(m for _, _, m in parts)
        x, inv = got_np(SW.region_rows(parts, gap, ranks=torch.tensor(ranks, device="cuda"), width=width))
        for r, row, bad in zip(ranks, x, inv):
            want, ok = SW.region_unrank(r, parts, gap)
            assert tuple(row[:k]) == want and bool(bad) == (not ok) and not row[k:].any(), (parts, r)

    # eight single bins of 200: T = 2.56e18 > 2^61, the 64-bit division in every part but the last few
    eight = [(1 + 200 * p, 201 + 200 * p, 1) for p in range(8)]
    T = SW.region_count(eight, 1)
    assert T == 200 ** 8 > 1 << 61
    near_top = [T - 1, T - 2, T - 200, T - 201, T - 200 ** 2, T - 200 ** 4 - 1, T - (1 << 32), T - (1 << 32) - 1, T // 2, T // 3, (1 << 61) + 12345,
                (1 << 32) - 1, 1 << 32, 200 ** 4, 200 ** 4 - 1, 1, 0]
    check(eight, 1, near_top)
    check(eight, 2, near_top)                                            # adjacent regions touch: the last of one and the first of the next are 1 apart
    x, inv = got_np(SW.region_rows(eight, 1, rank0=T - 1000, count=1000))
    assert tuple(x[-1]) == tuple(200 + 200 * p for p in range(8)) and not inv.any()
    assert (np.diff(x[:, 7]) == 1)[x[:-1, 7] != 1600].all()              # the last digit counts up and wraps at 200
    with pytest.raises(IndexError):
        SW.region_rows(eight, 1, rank0=T - 1, count=2)
    # a part of 4 with more than 2^40 candidates beside a single bin and a pair: unrank behind a 64-bit division
    mixed = [(1, 2492, 4), (3000, 3100, 1), (4000, 4007, 2)]
    T = SW.region_count(mixed, 2)
    assert T > 1 << 50
    check(mixed, 2, [0, 1, T - 1, T // 2, T // 3 + 7, (1 << 40) + 12345, T - 1500, 1499], width=8)
    # around 2^32, where the decoder changes between the 32-bit and the 64-bit division part by part
    two = [(1, 70001, 1), (80000, 150000, 1)]
    T = SW.region_count(two, 1)
    assert 1 << 32 < T < 1 << 33
    check(two, 1, [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, T - 1, 69999, 70000, 70001, 0])


# ---- against the reference ---------------------------------------------------------------------------------------------------------
def fixture_cases():
    if "g18" not in _CACHE:
        g = gold("g18_regions_tiny.npz")
        cases = []
        for i, (case, gap) in enumerate(RR.CASES):
            parts = RR.case_parts(case, TINY)
            rows, bad = brute(parts, gap)
            cases.append(dict(i=i, parts=parts, gap=gap, rows=rows, bad=bad, k=rows.shape[1], n_invalid=int(g[f"ninvalid_c{i}"]),
                              ref={mode: g[f"logit_{mode}_c{i}"].astype(np.float64) for mode in ("table", "adj")},
                              ksel={mode: int(g[f"ksel_{mode}_c{i}"]) for mode in ("table", "adj")}))
        _CACHE["g18"] = cases
    return _CACHE["g18"]


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_region_sweep_against_reference_logits(mode):
    clf = load_tiny(mode)
    for case in fixture_cases():
        parts, gap, rows, bad, ref = case["parts"], case["gap"], case["rows"], case["bad"], case["ref"][mode]
        T, k = len(rows), case["k"]
        index = {tuple(r): j for j, r in enumerate(rows.tolist()) if not bad[j]}
        scale = float(np.abs(ref).max())
        K = case["ksel"][mode]
        valid_ranks = np.flatnonzero(~bad)
        want = set(valid_ranks[np.argsort(-ref[valid_ranks])[:K]].tolist())
        first = None
        for chunk_rows in (37, 10000):
            with _lib.launch_log() as log:
                out = SW.region_sweep(clf, parts, gap, top=T, chunk_rows=chunk_rows)
            chunks = -(-T // chunk_rows)
            assert log.counts[KERNEL] == chunks + 1 and log.counts["topk_merge_kernel"] == chunks and "kway_rows_kernel" not in log.counts
            assert "kway_anchor_rows_kernel" not in log.counts
            assert out["n_candidates"] == T and out["n_invalid"] == case["n_invalid"] == int(bad.sum()) and out["n_excluded"] == 0
            kept, logit, rank = out["rows"].cpu().numpy(), out["logit"].cpu().numpy(), out["rank"].cpu().numpy()
            assert kept.shape == (T - case["n_invalid"], k)              # every valid candidate, and nothing else
            where = np.asarray([index[tuple(r)] for r in kept.tolist()], dtype=np.int64)       # a valid fixture row (KeyError otherwise)
            assert np.array_equal(where, rank) and len(set(where.tolist())) == len(where)
            err = float(np.abs(logit.astype(np.float64) - ref[where]).max()) / scale
            print(f"case {case['i']} {mode} chunk_rows {chunk_rows}: {len(where)} kept, max |logit - reference| / max |reference| = {err:.2e}")
            assert err < TOL, (case["i"], mode, err)
            assert (logit[:-1] >= logit[1:]).all()
            assert set(where[:K].tolist()) == want, (case["i"], mode)    # the first K_sel kept rows as a set: the reference's top K_sel
            assert torch.equal(out["proba"], torch.sigmoid(out["logit"]))
            if first is None:
                first = out
            else:                                                        # the chunking is not part of the result
                assert all(torch.equal(out[key], first[key]) for key in ("rows", "logit", "proba", "rank"))
        short = SW.region_sweep(clf, parts, gap, top=K, chunk_rows=37)
        assert all(torch.equal(short[key], first[key][:K]) for key in ("rows", "logit", "proba", "rank"))


def check_leading_against_fixture(out, a, ids, case, ref, top):
    """One leading candidate of a per_leading result against the valid fixture rows that begin with ``ids``: count, membership, tolerance,
    descending order, and the empty tail zero / -1."""
    rows, bad = case["rows"], case["bad"]
    member = np.flatnonzero((rows[:, :len(ids)] == np.asarray(ids)).all(axis=1) & ~bad)
    index = {tuple(r): j for j, r in zip(member.tolist(), rows[member].tolist())}
    count = int(out["count"][a])
    assert count == min(top, len(member)), (ids, count, len(member))
    kept = out["rows"][a, :count].cpu().numpy()
    logit = out["logit"][a, :count].cpu().numpy()
    where = np.asarray([index[tuple(r)] for r in kept.tolist()], dtype=np.int64)
    assert len(set(where.tolist())) == count and np.array_equal(where, out["rank"][a, :count].cpu().numpy())
    if count:
        assert float(np.abs(logit.astype(np.float64) - ref[where]).max()) / float(np.abs(ref).max()) < TOL, ids
        assert (logit[:-1] >= logit[1:]).all()
    assert bool((out["rank"][a, count:] == -1).all()) and not out["rows"][a, count:].any() and not out["logit"][a, count:].any()
    assert not out["proba"][a, count:].any()


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_region_sweep_per_leading(mode):
    clf = load_tiny(mode)
    top = 16
    for case in fixture_cases()[:3]:                                     # cases i and ii; case iii for its invalid rows and a leading PAIR
        parts, gap, ref = case["parts"], case["gap"], case["ref"][mode]
        m0 = parts[0][2]
        lead_rows, _ = RR.candidates([(parts[0][0], parts[0][1], m0), (1 << 20, (1 << 20) + 1, 1)], gap)
        lead_rows = lead_rows[:, :m0]
        A, seg = len(lead_rows), len(case["rows"]) // len(lead_rows)
        first = None
        for chunk_rows in (37, 10000):
            with _lib.launch_log() as log:
                out = SW.region_sweep(clf, parts, gap, top=top, chunk_rows=chunk_rows, per_leading=True)
            chunks = -(-len(case["rows"]) // chunk_rows)
            assert log.counts["segtopk_merge_kernel"] == chunks and log.counts[KERNEL] == chunks + (1 if m0 == 1 else 2)
            assert "kway_rows_kernel" not in log.counts and "topk_merge_kernel" not in log.counts
            K = min(top, seg)
            assert out["rows"].shape == (A, K, case["k"]) and out["logit"].shape == out["proba"].shape == out["rank"].shape == (A, K)
            assert np.array_equal(out["leading"].cpu().numpy(), lead_rows) and out["count"].shape == (A,)
            assert out["n_candidates"] == len(case["rows"]) and out["n_invalid"] == case["n_invalid"] and out["n_excluded"] == 0
            for a in range(A):
                check_leading_against_fixture(out, a, lead_rows[a].tolist(), case, ref, top)
            kept = out["rank"] >= 0
            assert torch.equal(out["proba"][kept], torch.sigmoid(out["logit"][kept]))
            if first is None:
                first = out
            else:
                assert all(torch.equal(out[key], first[key]) for key in ("rows", "logit", "proba", "rank", "count", "leading"))
        if case["i"] == 2:
            assert int(out["count"].min()) < top                         # a leading pair next to the boundary has fewer valid partners
        if case["i"] == 0:
            # every bin of chr0 as a single anchor with pairs of chr2: the anchored sweep, row for row, logits bitwise (both pin the same
            # forward route at the same width)
            (a_lo, a_hi, _), (lo, hi, _) = parts
            anc = SW.anchored_sweep(clf, np.arange(a_lo, a_hi, dtype=np.int64), lo, hi, 3, gap, top=top)
            assert torch.equal(anc["rows"], first["rows"]) and torch.equal(anc["logit"], first["logit"]) and torch.equal(anc["count"], first["count"])
            assert torch.equal(anc["proba"], first["proba"]) and torch.equal(anc["rank"], first["rank"] - torch.arange(A, device="cuda").view(-1, 1) * seg)


# ---- pair maps ---------------------------------------------------------------------------------------------------------------------
def planes_np(out):
    return {name: out[name].cpu().numpy() for name in PLANES}


def same_planes(a, b):
    return all(np.array_equal(a[name].view(np.uint32) if name == "max" else a[name], b[name].view(np.uint32) if name == "max" else b[name])
               for name in PLANES)


def test_region_map_against_the_numpy_twin():
    clf = load_tiny("table")
    clf.eval()
    cases = fixture_cases()
    for case, r, c in ((cases[0], 0, 1), (cases[0], 1, 0), (cases[0], 1, 1), (cases[2], 1, 1), (cases[2], 0, 1), (cases[3], 0, 2)):
        parts, gap = case["parts"], case["gap"]
        x, flag = SW.region_rows(parts, gap)
        with torch.no_grad(), _lib.option("disable_small_batch"):
            value = torch.sigmoid(clf(x).reshape(-1)).cpu().numpy()      # the device's own probabilities and flags into the twin
        regions = [(parts[p][0], parts[p][1] - parts[p][0]) for p in (r, c)]
        ref = pairmap_ref(x.cpu().numpy(), value, regions[0], regions[1], skip=flag.cpu().numpy())
        ref["sum"] = ref["sum"] / SCALE
        assert ref["n_rows"] == len(x) - case["n_invalid"]
        if case["n_invalid"]:                                            # invalid rows contribute nothing: the map of the valid rows alone
            keep = ~case["bad"]
            assert np.array_equal(flag.cpu().numpy() != 0, case["bad"])
            alone = pairmap_ref(x.cpu().numpy()[keep], value[keep], regions[0], regions[1])
            alone["sum"] = alone["sum"] / SCALE
            assert same_planes(alone, ref) and alone["n_rows"] == ref["n_rows"]
        outs = []
        for chunk_rows in (37, None):
            with _lib.launch_log() as log:
                out = SW.region_map(clf, parts, gap, r, c, chunk_rows=chunk_rows)
            chunks = -(-len(x) // (chunk_rows or len(x)))
            assert log.counts["pairmap_update_kernel"] == chunks == log.counts[KERNEL] and log.counts["pairmap_init_kernel"] == 1
            assert out["n_candidates"] == len(x) and out["n_invalid"] == case["n_invalid"] and out["n_excluded"] == 0 and out["n_rejected"] == 0
            assert out["count"].shape == (regions[0][1], regions[1][1])
            assert same_planes(planes_np(out), ref), (case["i"], r, c, chunk_rows)
            outs.append(out)
        assert all(torch.equal(outs[0][name], outs[1][name]) for name in PLANES + ("mean",))
        cnt = outs[0]["count"].cpu().numpy()
        if case["n_invalid"] == 0 and r != c:                            # every candidate lands m_r m_c times
            assert cnt.sum() == len(x) * parts[r][2] * parts[c][2]
        assert cnt.max() <= SW.region_map_bound(parts, gap, r, c)
    # exclusion and the transpose
    case = cases[0]
    hset = HyperedgeSet(torch.from_numpy(case["rows"][:100].copy()).cuda())
    exc = SW.region_map(clf, case["parts"], case["gap"], 0, 1, exclude=hset, chunk_rows=37)
    full = SW.region_map(clf, case["parts"], case["gap"], 0, 1)
    flip = SW.region_map(clf, case["parts"], case["gap"], 1, 0)
    assert exc["n_excluded"] == 100 and int(exc["count"].sum()) == int(full["count"].sum()) - 200
    assert all(torch.equal(flip[name], full[name].t()) for name in PLANES)
    only = SW.region_map(clf, case["parts"], case["gap"], 0, 1, planes=["max"])
    assert set(only) == {"max", "n_candidates", "n_invalid", "n_excluded", "n_rejected"} and torch.equal(only["max"], full["max"])
    # the capacity refusal fires before any launch
    huge = [(1, 60001, 1), (70000, 140000, 2), (150000, 210000, 1)]
    with _lib.launch_log() as log:
        with pytest.raises(ValueError, match="capacity"):
            SW.region_map(clf, huge, 1, 0, 2)
        empty = SW.region_map(clf, [(1, 7, 3), (40, 56, 2)], 4, 0, 1)    # T = 0: empty planes, nothing launched
    assert not log.counts and empty["n_candidates"] == 0 and empty["count"].shape == (6, 16) and not empty["count"].any()
    assert bool(torch.isinf(empty["max"]).all())


# ---- three chromosomes, d = 64 -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trans3():
    """The d = 64 table model of tests/test_hip_kway.py's d64, three windows of 10 bins on three chromosomes of hg38 at 1 Mb with one
    bin drawn from each: 1 000 candidates, and ``full`` = model(all rows) in one batch ON THE PINNED ROUTE at widths 3 and 5 (a batch
    of 1 000 would otherwise take the small-batch forward, which rounds a few ulp differently: tests/test_hip_kanchor.py's trans)."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    cr = np.asarray(synth.chrom_range(num))
    clf, _ = hip_model(num, 64, "table", 12)
    clf.eval()
    parts = [(int(cr[0][0]) + 10, int(cr[0][0]) + 20, 1), (int(cr[5][0]) + 3, int(cr[5][0]) + 13, 1), (int(cr[10][0]) + 40, int(cr[10][0]) + 50, 1)]
    rows, bad = brute(parts, 3)
    assert len(rows) == 1000 and not bad.any()
    full = {}
    with torch.no_grad(), _lib.option("disable_small_batch"):
        for width in (3, 5):
            x = torch.from_numpy(np.pad(rows, ((0, 0), (0, width - 3)))).cuda()
            full[width] = clf(x).reshape(-1).clone()
    return dict(clf=clf, parts=parts, rows=rows, full=full, N=int(np.sum(num)), cr=cr)


def check_region_top(out, full, rows, parts, width, top, candidates=None):
    """check_top's properties (tests/test_hip_kway.py) for a region sweep."""
    rank = out["rank"]
    assert rank.numel() == top and len(set(rank.tolist())) == top
    assert float((out["logit"] - full[rank]).abs().max()) <= 1e-6        # what two batchings of one forward may differ by
    assert bool((out["logit"][:-1] >= out["logit"][1:]).all())
    got_rows = out["rows"].cpu().numpy()
    assert got_rows.shape == (top, width) and not got_rows[:, 3:].any()
    for r, row in zip(rank.tolist()[::9], got_rows[::9]):
        assert SW.region_unrank(r, parts, 3) == (tuple(row[:3]), True)
    assert np.array_equal(got_rows[:, :3], rows[rank.cpu().numpy()])
    left = torch.ones(full.numel(), dtype=torch.bool, device=full.device)
    if candidates is not None:
        left[:] = False
        left[candidates] = True
        assert bool(left[rank].all())                                    # no winner from outside the eligible ranks
    left[rank] = False
    assert float(full[left].max()) <= float(out["logit"].min()) + 2e-6   # nobody left out beats the last winner


@pytest.mark.parametrize("chunk_rows", [333, 1 << 20])
def test_region_sweep_three_chromosomes_d64(trans3, chunk_rows):
    clf, parts, rows, full = trans3["clf"], trans3["parts"], trans3["rows"], trans3["full"]
    out = SW.region_sweep(clf, parts, 3, top=100, chunk_rows=chunk_rows)
    assert out["n_candidates"] == 1000 and out["n_invalid"] == 0 and out["n_excluded"] == 0 and out["rows"].is_cuda
    check_region_top(out, full[3], rows, parts, 3, 100)
    assert torch.equal(out["proba"], torch.sigmoid(out["logit"]))
    wide = SW.region_sweep(clf, parts, 3, top=100, chunk_rows=chunk_rows, width=5)
    check_region_top(wide, full[5], rows, parts, 5, 100)
    assert float((full[5] - full[3]).abs().max()) > 1e-4                 # the width is part of the result (pads are attended)


def test_region_sweep_exclude_regress_empty_and_bad_ids(trans3):
    clf, parts, rows, full = trans3["clf"], trans3["parts"], trans3["rows"], trans3["full"]
    everything = SW.region_sweep(clf, parts, 3, top=100)
    winners = everything["rank"].cpu().numpy()[::3]                      # some of the winners become known hyperedges
    hset = HyperedgeSet(torch.from_numpy(rows[winners]).cuda())
    out = SW.region_sweep(clf, parts, 3, top=100, chunk_rows=333, exclude=hset)
    assert out["n_excluded"] == len(winners) and out["n_invalid"] == 0 and out["n_candidates"] == 1000
    assert not np.isin(out["rank"].cpu().numpy(), winners).any()
    rest = torch.from_numpy(np.setdiff1d(np.arange(1000), winners)).cuda()
    check_region_top(out, full[3], rows, parts, 3, 100, candidates=rest)
    reg = SW.region_sweep(clf, parts, 3, top=100, task_mode="regress")
    assert torch.equal(reg["rank"], everything["rank"]) and torch.equal(reg["proba"], torch.nn.functional.softplus(reg["logit"]))
    # top larger than T: every candidate that is not excluded, once
    small = [(lo, lo + 3, m) for lo, _, m in parts]
    all_of = SW.region_sweep(clf, small, 3, top=1000)
    assert all_of["n_candidates"] == 27 and sorted(all_of["rank"].tolist()) == list(range(27))
    per = SW.region_sweep(clf, small, 3, top=1000, per_leading=True)
    assert per["rows"].shape == (3, 9, 3) and bool((per["count"] == 9).all()) and per["leading"].view(-1).tolist() == [parts[0][0] + j for j in range(3)]
    assert sorted(per["logit"].view(-1).tolist()) == sorted(all_of["logit"].tolist())
    # T = 0: a part too small for its bins; nothing is launched
    none = [parts[0], (parts[1][0], parts[1][0] + 4, 3), parts[2]]
    with _lib.launch_log() as log:
        empty = SW.region_sweep(clf, none, 3, top=100)
        empty_per = SW.region_sweep(clf, none, 3, top=100, per_leading=True)
    assert not log.counts and empty["n_candidates"] == 0 and empty["rows"].shape == (0, 5)
    assert all(empty[key].numel() == 0 and empty[key].is_cuda for key in ("logit", "proba", "rank"))
    assert empty_per["rows"].shape == (0, 0, 5) and empty_per["count"].shape == (0,) and empty_per["leading"].shape == (0, 1)
    # an id beyond the model's tables: raised once, at the end
    N = trans3["N"]
    with pytest.raises(IndexError):
        SW.region_sweep(clf, parts[:2] + [(N - 4, N + 6, 1)], 3, top=10)
    with pytest.raises(IndexError):
        SW.region_map(clf, parts[:2] + [(N - 4, N + 6, 1)], 3, 0, 2)
    assert clf.check_ids                                                 # the per-call check is back on
    again = SW.region_sweep(clf, parts, 3, top=100)
    assert all(torch.equal(again[key], everything[key]) for key in ("rows", "logit", "proba", "rank"))


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_region_cli(tmp_path):
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
    out = os.path.join(tmp_path, "regions.tsv")
    spec = ["--part", "0:1:0-8", "--part", "%s:1:0-8" % names[1], "--part", "3:2:8-16"]       # the fixture's case ii; min_gap = min_distance + 1 = 2
    parts = RR.case_parts(RR.CASES[1][0], cr)
    clf = load_tiny("table")

    def run(*extra):
        PR.main(["regions", *spec, "-o", out, "--config", cpath, *extra])
        return np.load(os.path.join(tmp_path, "regions.npz")), [line.rstrip("\n").split("\t") for line in open(out)]

    # a list
    z, lines = run("--top", "20")
    ref = SW.region_sweep(clf, parts, 2, top=20)
    assert set(z.files) == {"rows", "logit", "proba", "rank"} and len(lines) == 20
    assert all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in ("rows", "logit", "proba", "rank"))
    for line, row, p in zip(lines, z["rows"], z["proba"]):
        assert [bin2node[item] for item in line[:4]] == row.tolist() and np.float32(float(line[4])) == p
        assert [item.split(":")[0] for item in line[:4]] == [names[0], names[1], names[3], names[3]]
    # --exclude-known drops the rows of all_4_counter.npy: the winners move up
    np.save(os.path.join(temp, "all_4_counter.npy"), z["rows"][[0, 3, 4]])
    e, _ = run("--top", "20", "--exclude-known")
    more = SW.region_sweep(clf, parts, 2, top=23)["rows"].cpu().numpy()
    assert np.array_equal(e["rows"], more[[i for i in range(23) if i not in (0, 3, 4)]])
    # --per-leading: grouped by the bin of the first part, best first
    z, lines = run("--top", "5", "--per-leading", "--min-gap", "3", "--chunk-rows", "100")
    ref = SW.region_sweep(clf, parts, 3, top=5, per_leading=True)
    assert set(z.files) == {"rows", "logit", "proba", "rank", "count", "leading"} and z["rows"].shape == (8, 5, 4)
    assert all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in ("rows", "logit", "proba", "rank", "count", "leading"))
    assert len(lines) == int(z["count"].sum()) == 40
    at = 0
    for a in range(8):
        for row, p in zip(z["rows"][a, :z["count"][a]], z["proba"][a, :z["count"][a]]):
            assert [bin2node[item] for item in lines[at][:4]] == row.tolist() and np.float32(float(lines[at][4])) == p and row[0] == z["leading"][a, 0]
            at += 1
    # --map R C: the planes instead of a list
    z, _ = run("--map", "0", "2", "--threshold", "0.25")
    ref = SW.region_map(clf, parts, 2, 0, 2, threshold=0.25)
    assert {"sum", "mean", "max", "count", "count_ge", "parts", "rows_part", "cols_part"} <= set(z.files) and z["count"].shape == (8, 8)
    assert all(np.array_equal(z[name], ref[name].cpu().numpy()) for name in PLANES + ("mean",)) and np.array_equal(z["parts"], np.asarray(parts))
    with pytest.raises(ValueError, match=r"--part 0:1"):
        PR.main(["regions", "--part", "2:1", "--part", "0:1", "--top", "5", "-o", out, "--config", cpath])
