"""Pair maps on the MI355X (csrc/pairmap.hip, matcha_amd/sweep.py): every plane bit for bit against the numpy restatement
(tests/pairmap_ref.py) for any row order and any cutting of the stream; kway_map against the reference's own logits (g11), against
kway_sweep and against the restatement fed the device's values; the refusals; the CLI."""
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
from tests.helpers import GOLD, gold
from tests.pairmap_ref import SCALE, golden_cut, pairmap_ref, sigmoid64
from tests.test_cpu_kway import brute
from tests.test_hip_kway import load_tiny

pytestmark = pytest.mark.gpu

TOL = 1e-4                       # the device forward against the reference's CPU logits (tests/test_hip_kway.py)
PLANES = ("sum", "count", "count_ge", "max")
SPECIALS = [0.0, 1.0, -0.0, 1e-45, 2.0 ** -40, np.nan, -1.0, 1.5, np.inf, 0.5]
REGIONS = {"sym7": ((3, 7), (3, 7)), "sym300": ((1, 300), (1, 300)), "rect": ((1, 5), (40, 9))}


def make_case(n, L, regions, seed, ordered):
    """n rows of mixed sizes 2 .. L, zero-padded (a few with a zero in the middle), ids from both regions and from outside them, repeated
    ids inside a row; values in [0, 1] salted with SPECIALS (each in a kept and in a skipped row); a random skip mask.  ``ordered``: rows in lexicographic order."""
    rng = np.random.default_rng(seed)
    (lo_r, n_r), (lo_c, n_c) = regions
    pool = np.concatenate([np.arange(lo_r, lo_r + n_r), np.arange(lo_c, lo_c + n_c), [lo_r + n_r, lo_c + n_c + 3, 10000, 1 << 40]])
    if lo_r > 1:
        pool = np.append(pool, lo_r - 1)
    x = rng.choice(pool, (n, L)).astype(np.int64)
    dup = rng.random(n) < 0.1
    x[dup, 1] = x[dup, 0]
    size = rng.integers(2, L + 1, n)
    x[np.arange(L)[None, :] >= size[:, None]] = 0
    hole = rng.random(n) < 0.05
    x[hole, rng.integers(0, L, n)[hole]] = 0
    if ordered:
        x = x[np.lexsort(x.T[::-1])]
    v = rng.random(n).astype(np.float32)
    skip = ((rng.random(n) < 0.15) * rng.integers(1, 5, n)).astype(np.int32)
    where = rng.permutation(n)[:2 * len(SPECIALS)]                       # every special value once kept and once skipped
    v[where] = np.asarray(SPECIALS + SPECIALS, dtype=np.float32)[:len(where)]
    skip[where] = np.repeat([0, 2], len(SPECIALS))[:len(where)]
    return x, v, skip


def run_map(x, v, skip, regions, planes="all", pieces=None, vmax=1.0, threshold=0.5):
    pm = SW.PairMap(regions[0], regions[1], planes, vmax=vmax, threshold=threshold)
    xt, vt = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    kt = None if skip is None else torch.from_numpy(skip).cuda()
    piece = len(x) if pieces is None else pieces
    for a in range(0, len(x), piece):
        pm.update(xt[a:a + piece], vt[a:a + piece], None if kt is None else kt[a:a + piece])
    return {key: t.cpu().numpy() for key, t in pm.read().items()}


def assert_same(got, ref, names=PLANES):
    for name in names:
        a, b = got[name], ref[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if name == "max":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    assert got["counters"].tolist() == [ref["n_rows"], ref["n_rejected"]]


# ---- exactness against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", sorted(REGIONS))
def test_every_plane_bitwise_equal_to_the_restatement(region):
    regions = REGIONS[region]
    seed = 0
    for n in (1, 63, 64, 65, 257, 4099):
        for L in (2, 3, 5, 8):
            for ordered in (True, False):
                seed += 1
                x, v, skip = make_case(n, L, regions, seed, ordered)
                use_skip = skip if seed % 3 else None
                ref = pairmap_ref(x, v, regions[0], regions[1], skip=use_skip)
                with _lib.launch_log() as log:
                    got = run_map(x, v, use_skip, regions)
                assert log.counts == {"pairmap_init_kernel": 1, "pairmap_update_kernel": 1, "pairmap_read_kernel": 4}
                assert_same(got, ref)
                if n == 4099:
                    assert ref["n_rejected"] >= 4 and ref["count"].max() > 1 and np.isinf(ref["max"]).sum() < ref["max"].size
    if region == "sym7":                                                 # everything lands on 21 cells
        assert (ref["count"][np.triu_indices(7, 1)] > 50).all()


@pytest.mark.parametrize("planes", [["sum"], ["count"], ["count_ge"], ["max"], ["sum", "max"], 6])
def test_plane_masks(planes):
    names = [p for p in PLANES if _lib.PAIRMAP_PLANES[p] & planes] if isinstance(planes, int) else planes
    for region, L in (("sym7", 3), ("sym300", 5), ("rect", 8)):
        regions = REGIONS[region]
        x, v, skip = make_case(4099, L, regions, 77, True)
        ref = pairmap_ref(x, v, regions[0], regions[1], skip=skip)
        with _lib.launch_log() as log:
            got = run_map(x, v, skip, regions, planes=planes)
        assert log.counts["pairmap_read_kernel"] == len(names) and log.counts["pairmap_update_kernel"] == 1
        assert set(got) == set(names) | {"counters"}
        assert_same(got, ref, names)


def test_vmax_and_threshold_are_part_of_the_contract():
    regions = REGIONS["sym7"]
    x, v, skip = make_case(257, 3, regions, 5, True)
    v = (v * np.float32(3.0)).astype(np.float32)                         # values up to 3, 1.5 * 3 = 4.5 among them
    for vmax, threshold in ((2.0, 0.25), (4.5, 1.0), (float(2 ** 20), 3.0)):
        ref = pairmap_ref(x, v, regions[0], regions[1], vmax=vmax, threshold=threshold, skip=skip)
        assert_same(run_map(x, v, skip, regions, vmax=vmax, threshold=threshold), ref)
    big = np.full(64, 2.0 ** 20, dtype=np.float32)
    rows = np.tile(np.asarray([[3, 4]], dtype=np.int64), (64, 1))
    got = run_map(rows, big, None, regions, vmax=float(2 ** 20))
    assert got["sum"][0, 1] == 64 << 52 and got["max"][0, 1] == 2.0 ** 20 and got["counters"].tolist() == [64, 0]


def test_one_cell_takes_everything():
    regions = REGIONS["sym300"]
    for row in ([3, 5], [5, 3, 0], [3, 3, 5]):
        x = np.tile(np.asarray([row], dtype=np.int64), (100000, 1))
        v = np.ones(100000, dtype=np.float32)
        with _lib.launch_log() as log:
            got = run_map(x, v, None, regions)
        assert log.counts["pairmap_update_kernel"] == 1
        times = 2 if row == [3, 3, 5] else 1                             # one contribution per pair of positions
        assert got["sum"][2, 4] == got["sum"][4, 2] == times * 100000 << 32
        assert got["count"][2, 4] == got["count_ge"][2, 4] == times * 100000 and got["max"][2, 4] == 1.0
        assert got["count"].sum() == 2 * times * 100000 and got["counters"].tolist() == [100000, 0]


def test_planes_do_not_depend_on_how_the_stream_is_cut():
    for region, L in (("sym7", 3), ("sym300", 8), ("rect", 5)):
        regions = REGIONS[region]
        x, v, skip = make_case(4099, L, regions, 31, True)
        ref = pairmap_ref(x, v, regions[0], regions[1], skip=skip)
        for piece in (1, 37, 64, 4099):
            assert_same(run_map(x, v, skip, regions, pieces=piece), ref)


def test_update_takes_anchored_rows_and_rows_of_different_widths():
    lo, n = 2, 20
    anchors = torch.tensor([[4], [11], [30]], device="cuda")
    x, flag = SW.anchored_rows(anchors, lo, n, 3, 2)
    rng = np.random.default_rng(9)
    v = rng.random(len(x)).astype(np.float32)
    assert 0 < int((flag != 0).sum()) < len(x)
    pm = SW.PairMap((lo, n), (lo, n))
    pm.update(x, torch.from_numpy(v).cuda(), flag)
    wide = np.asarray([[2, 9, 21, 0, 0], [21, 20, 19, 18, 17]], dtype=np.int64)          # a second update of another width, unsorted ids
    pm.update(torch.from_numpy(wide).cuda(), torch.tensor([0.75, 0.5], device="cuda"))
    got = {key: t.cpu().numpy() for key, t in pm.read().items()}
    a = pairmap_ref(x.cpu().numpy(), v, (lo, n), (lo, n), skip=flag.cpu().numpy())
    b = pairmap_ref(wide, np.asarray([0.75, 0.5], dtype=np.float32), (lo, n), (lo, n))
    ref = {name: a[name] + b[name] for name in ("sum", "count", "count_ge", "n_rows", "n_rejected")}
    ref["max"] = np.maximum(a["max"], b["max"])
    assert_same(got, ref)
    out = pm.result()
    assert out["sum"].dtype == torch.float64 and np.array_equal(out["sum"].cpu().numpy(), ref["sum"] / SCALE)
    mean = np.where(ref["count"] > 0, ref["sum"] / SCALE / np.maximum(ref["count"], 1), 0.0).astype(np.float32)
    assert out["mean"].dtype == torch.float32 and np.array_equal(out["mean"].cpu().numpy(), mean)
    assert int(out["n_rows"]) == ref["n_rows"] and int(out["n_rejected"]) == 0
    with pytest.raises(ValueError):
        pm.update(x.to(torch.int32), torch.from_numpy(v).cuda())
    with pytest.raises(_lib.MatchaHipError):
        pm.update(torch.zeros(4, 9, dtype=torch.long, device="cuda"), torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        SW.PairMap((1, 7), (3, 7))                                       # overlapping, not equal


# ---- against the reference's logits --------------------------------------------------------------------------------------------------
def g11_case(g, i):
    cr = np.asarray(synth.chrom_range([int(v) for v in g["num"]]))
    c, k, gap = (int(v) for v in g["cases"][i])
    return int(cr[c][0]), int(cr[c][1]), k, gap


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_map_against_reference_logits(mode):
    g = gold("g11_kway_tiny.npz")
    clf = load_tiny(mode)
    for i in range(3):
        lo, hi, k, gap = g11_case(g, i)
        n = hi - lo
        rows, logit = g[f"rows_c{i}"], g[f"logit_{mode}_c{i}"].astype(np.float64)
        assert np.array_equal(rows, np.asarray(brute(lo, n, k, gap), dtype=np.int64))
        cut, _ = golden_cut(logit)
        threshold = float(np.float32(sigmoid64(cut)))
        p = sigmoid64(logit)
        cnt, s64, ge = np.zeros((n, n), dtype=np.int64), np.zeros((n, n)), np.zeros((n, n), dtype=np.int64)
        m64 = np.full((n, n), -np.inf)
        for ci, cj in itertools.combinations(range(k), 2):
            for a, b in ((ci, cj), (cj, ci)):
                np.add.at(cnt, (rows[:, a] - lo, rows[:, b] - lo), 1)
                np.add.at(s64, (rows[:, a] - lo, rows[:, b] - lo), p)
                np.add.at(ge, (rows[:, a] - lo, rows[:, b] - lo), (logit > cut).astype(np.int64))
                np.maximum.at(m64, (rows[:, a] - lo, rows[:, b] - lo), p)
        with _lib.launch_log() as log:
            out = SW.kway_map(clf, lo, hi, k, gap, threshold=threshold)
        assert log.counts["pairmap_update_kernel"] == 1 and log.counts["kway_rows_kernel"] == 1 and log.counts["pairmap_read_kernel"] == 4
        assert out["n_candidates"] == len(rows) and out["n_excluded"] == 0 and out["n_rejected"] == 0
        got = {name: out[name].cpu().numpy() for name in PLANES + ("mean",)}
        assert np.array_equal(got["count"], cnt)
        per = TOL * np.abs(logit).max() / 4 + 2.0 ** -33
        err_sum, err_max = np.abs(got["sum"] - s64), np.abs(np.where(cnt > 0, got["max"].astype(np.float64) - np.where(cnt > 0, m64, 0), 0))
        print(f"{mode} case {i}: sum error / bound {np.max(err_sum / np.maximum(cnt * per, 1e-300)):.3g}, max error / bound {err_max.max() / per:.3g}")
        assert (err_sum <= cnt * per).all() and (err_max <= per).all()
        assert np.isneginf(got["max"][(cnt == 0) & ~np.eye(n, dtype=bool)]).all() and not np.diag(got["max"]).any()
        assert np.array_equal(got["count_ge"], ge), (mode, i)
        assert 0 < ge.sum() < cnt.sum()


# ---- ties to what exists -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The reference's tiny table model, the first g11 case (k = 3, 560 candidates), and the device's own value of every candidate:
    sigmoid of one forward over all rows on the sweep's kernel route."""
    g = gold("g11_kway_tiny.npz")
    clf = load_tiny("table")
    clf.eval()
    lo, hi, k, gap = g11_case(g, 0)
    rows = g["rows_c0"]
    with torch.no_grad(), _lib.option("disable_small_batch"):
        value = torch.sigmoid(clf(torch.from_numpy(rows).cuda()).reshape(-1)).cpu().numpy()
    full = SW.kway_map(clf, lo, hi, k, gap)
    return dict(clf=clf, lo=lo, hi=hi, k=k, gap=gap, rows=rows, value=value, full=full, N=int(np.sum(g["num"])))


def planes_np(out):
    return {name: out[name].cpu().numpy() for name in PLANES}


def same_planes(a, b):
    return all(np.array_equal(a[name].view(np.uint32) if name == "max" else a[name], b[name].view(np.uint32) if name == "max" else b[name])
               for name in PLANES)


def ref_planes(rows, value, region, cols=None, skip=None):
    ref = pairmap_ref(rows, value, region, cols or region, skip=skip)
    ref["sum"] = ref["sum"] / SCALE
    return ref


def test_map_ties_to_sweep_chunks_exclusion_and_windows(tiny):
    clf, lo, hi, k, gap, rows, value = (tiny[key] for key in ("clf", "lo", "hi", "k", "gap", "rows", "value"))
    n = hi - lo
    full = planes_np(tiny["full"])
    assert same_planes(full, ref_planes(rows, value, (lo, n)))           # the map is the restatement of the device's own values
    best = SW.kway_sweep(clf, lo, hi, k, gap, top=1)
    top = torch.sigmoid(best["logit"]).cpu().numpy().view(np.uint32)[0]
    assert full["max"].max().view(np.uint32) == top
    r = best["rows"].cpu().numpy()[0] - lo
    assert full["max"][r[0], r[1]].view(np.uint32) == top == full["max"][r[2], r[1]].view(np.uint32)
    with _lib.launch_log() as log:
        cut = SW.kway_map(clf, lo, hi, k, gap, chunk_rows=37)
    assert log.counts["pairmap_update_kernel"] == -(-len(rows) // 37) and log.counts["pairmap_init_kernel"] == 1
    assert same_planes(planes_np(cut), full) and np.array_equal(cut["mean"].cpu().numpy(), tiny["full"]["mean"].cpu().numpy())
    hset = HyperedgeSet(torch.from_numpy(rows[:100]).cuda())
    for chunk_rows in (1 << 20, 37):
        exc = SW.kway_map(clf, lo, hi, k, gap, exclude=hset, chunk_rows=chunk_rows)
        assert exc["n_excluded"] == 100 and exc["n_candidates"] == len(rows) and exc["n_rejected"] == 0
        assert same_planes(planes_np(exc), ref_planes(rows[100:], value[100:], (lo, n)))
    assert not same_planes(planes_np(exc), full)
    for rw, cw in (((lo, 5), (lo + 8, 6)), ((lo + 8, 6), (lo, 5)), ((lo + n - 3, 3), (lo + 1, 4))):
        with _lib.launch_log() as log:
            rect = SW.kway_map(clf, lo, hi, k, gap, row_window=rw, col_window=cw)
        assert log.counts["pairmap_update_kernel"] == 1
        block = {name: full[name][rw[0] - lo:rw[0] - lo + rw[1], cw[0] - lo:cw[0] - lo + cw[1]] for name in PLANES}
        assert rect["count"].shape == (rw[1], cw[1]) and same_planes(planes_np(rect), block)
    # one plane only; a wider batch is another forward (pads are attended), so another map
    only = SW.kway_map(clf, lo, hi, k, gap, planes=["max"])
    assert set(only) == {"max", "n_candidates", "n_excluded", "n_rejected"} and torch.equal(only["max"], tiny["full"]["max"])
    wide = SW.kway_map(clf, lo, hi, k, gap, width=5)
    assert torch.equal(wide["count"], tiny["full"]["count"]) and not torch.equal(wide["sum"], tiny["full"]["sum"])


def test_map_regress_rejects_values_above_value_max(tiny):
    clf, lo, hi, k, gap, rows = (tiny[key] for key in ("clf", "lo", "hi", "k", "gap", "rows"))
    n = hi - lo
    with torch.no_grad(), _lib.option("disable_small_batch"):
        value = torch.nn.functional.softplus(clf(torch.from_numpy(rows).cuda()).reshape(-1)).cpu().numpy()
    vmax = float(np.sort(value)[400])
    out = SW.kway_map(clf, lo, hi, k, gap, task_mode="regress", value_max=vmax, threshold=vmax / 2)
    assert out["n_rejected"] == int((value > np.float32(vmax)).sum()) > 100
    ref = pairmap_ref(rows, value, (lo, n), (lo, n), vmax=vmax, threshold=vmax / 2)
    ref["sum"] = ref["sum"] / SCALE
    assert same_planes(planes_np(out), ref)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_map_refusals_and_empty_region(tiny):
    clf, lo, hi, k, gap, N = (tiny[key] for key in ("clf", "lo", "hi", "k", "gap", "N"))
    with pytest.raises(IndexError):
        SW.kway_map(clf, N - 10, N + 10, 3, 1)                           # a region beyond the model's tables: raised once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    with _lib.launch_log() as log:
        with pytest.raises(ValueError, match="capacity"):
            SW.kway_map(clf, 1, 120001, 5, 1)                            # C(m, 3) candidates per cell: past 2^31
        with pytest.raises(ValueError, match="value_max"):
            SW.kway_map(clf, lo, hi, k, gap, task_mode="regress")
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, task_mode="regress", value_max=float(2 ** 21))
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, task_mode="other")
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, row_window=(lo, 5))         # one window without the other
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, row_window=(lo, 5), col_window=(lo + 4, 5))     # overlapping windows
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, row_window=(lo, 5), col_window=(hi - 2, 5))     # outside the region
        with pytest.raises(ValueError):
            SW.kway_map(clf, lo, hi, k, gap, planes=["median"])
        empty = SW.kway_map(clf, lo, lo + 2, 3, 1)                       # two bins, k = 3: no candidates
    assert not log.counts
    assert empty["n_candidates"] == 0 and empty["n_excluded"] == 0 and empty["n_rejected"] == 0
    assert all(empty[name].shape == (2, 2) and empty[name].is_cuda and not empty[name].any() for name in ("sum", "count", "count_ge", "mean"))
    assert empty["max"].cpu().tolist() == [[0.0, -np.inf], [-np.inf, 0.0]]
    again = SW.kway_map(clf, lo, hi, k, gap)
    assert all(torch.equal(again[name], tiny["full"][name]) for name in PLANES + ("mean",))


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_kmap(tmp_path):
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
    out = os.path.join(tmp_path, "map.npz")

    def run(*extra):
        PR.main(["kmap", "--chrom", "2", "--k", "3", "-o", out, "--config", cpath, *extra])
        z = np.load(out)
        assert set(z.files) == {"sum", "mean", "max", "count", "count_ge", "lo", "n", "k", "min_gap", "threshold"}
        return z

    def check(z, ref, lo, n, threshold):
        assert (int(z["lo"]), int(z["n"]), int(z["k"]), int(z["min_gap"])) == (lo, n, 3, 2) and z["threshold"] == np.float32(threshold)
        for name in PLANES + ("mean",):
            a, b = z[name], ref[name].cpu().numpy()
            assert a.shape == (n, n) and a.dtype == b.dtype, name
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) if name == "max" else np.array_equal(a, b), name

    lo, hi = int(cr[2][0]), int(cr[2][1])
    clf = load_tiny("table")
    check(run(), SW.kway_map(clf, lo, hi, 3, 2), lo, hi - lo, 0.5)      # min_gap = min_distance + 1
    check(run("--start-bin", "2", "--end-bin", "12", "--threshold", "0.3"), SW.kway_map(clf, lo + 2, lo + 12, 3, 2, threshold=0.3), lo + 2, 10, 0.3)
    known = np.asarray(brute(lo, hi - lo, 3, 2), dtype=np.int64)[[0, 3, 4]]
    np.save(os.path.join(temp, "all_3_counter.npy"), known)
    e = run("--exclude-known")
    ref = SW.kway_map(clf, lo, hi, 3, 2, exclude=HyperedgeSet(torch.from_numpy(known).cuda()))
    assert ref["n_excluded"] == 3
    check(e, ref, lo, hi - lo, 0.5)
    assert e["count"].sum() == SW.kway_map(clf, lo, hi, 3, 2)["count"].sum().item() - 3 * 6
