"""Per-pair support on the MI355X (csrc/sweep_support.hip's subset_pair_update_kernel, matcha_amd/sweep.py's SubsetPairSupport and
decomposition_sweep(pair_support=True)): the packed planes bit for bit against the numpy twin (tests/pair_support_ref.py),
whatever the cut and the order, and in exact identities against the per-locus planes filled on the device from the same stream; the sweep's
pair matrices against the reference's own logits (g16); the untouched defaults; the CLI."""
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
from tests import denoise_ref as R
from tests import pair_support_ref as PS
from tests import subsets_ref as SR
from tests.helpers import GOLD, gold
from tests.test_cpu_pair_support import PAIR_CASES, g16_pair_reference
from tests.test_cpu_subsets import g16_case
from tests.test_hip_kway import load_tiny

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
PAIR = "subset_pair_update_kernel"
SUPPORT = "subset_support_update_kernel"
PAIR_KERNELS = {PAIR, "subset_pair_init_kernel", "subset_pair_read_kernel"}
PAIR_KEYS = ("pair_sum", "pair_count", "pair_mean")
OLD_KEYS = ("rows", "logit", "proba", "rank", "count", "chosen", "support_sum", "support_count", "support_mean")
DROP_ONLY = ("full_logit", "full_proba")


def planes_np(sup):
    z = sup.read()
    return z["sum"].cpu().numpy(), z["count"].cpu().numpy(), z["counters"].cpu().tolist()


def awkward_values(rng, n):
    """float32 values in [0, 1] with rejected ones (NaN, negative, too large, +-inf), -0.0 and exact ends, and a skip mask."""
    v = rng.random(n).astype(np.float32)
    at = rng.permutation(n)[:12]
    v[at] = [np.nan, -1e-3, 1.0000001, np.inf, -0.0, 0.0, 1.0, 1e-12, -np.inf, 2.0, 0.5, np.nan]
    skip = rng.random(n) < 0.15
    skip[at[:2]] = False
    skip[at[2]] = True                                                   # a skipped row is not rejected, whatever its value
    return v, skip


@pytest.mark.parametrize("A,S,m", [(60, 9, 3), (5000, 3, 2), (12, 32, 2), (4, 32, 3), (40, 8, 8), (3, 12, 8), (1000, 4, 3), (700, 5, 3)])
def test_pair_planes_bitwise(A, S, m):
    """The kernel's LDS tile holds 2 048 cells per plane and a block's run is 2 048 consecutive ranks.  (60, 9, 3): P = 36, a run spans 25
    or 26 clusters, inside the tile of 2 048 / 36 = 56; (5 000, 3, 2) and (12, 32, 2): m = 2, the direct path -- a row's cell is its global
    rank, no tile -- at P = 3 and P = 496; (4, 32, 3): C = 4 960, a run lies inside one cluster of 496 cells or across two, the tile holds
    4; (40, 8, 8): one choice per cluster, 28 cells per row, all 40 clusters in one run and in the tile of 73; (3, 12, 8): 495 choices,
    28 cells per row, P = 66; (1 000, 4, 3): C = 4 and P = 6, a run spans 512 clusters, the tile holds 341 and the rest goes to global
    atomics; (700, 5, 3): C = P = 10, a run spans 205 or 206 clusters, one or two more than the tile's 204."""
    cm = math.comb(S, m)
    n = A * cm
    rng = np.random.default_rng(A + S + m)
    v, skip = awkward_values(rng, n)
    want_sum, want_cnt, want_counters = PS.pair_support(A, S, m, v, skip, 0)
    vd, sd = torch.from_numpy(v).cuda(), torch.from_numpy(skip).cuda()
    first = None
    for chunk in (n, 37, 4099):
        sup = SW.SubsetPairSupport(A, S, m, device="cuda")
        with _lib.launch_log() as log:
            for g0 in range(0, n, chunk):
                sup.update(vd[g0:g0 + chunk], g0, sd[g0:g0 + chunk])
        assert log.counts == {PAIR: -(-n // chunk)}                      # its own kernel only, once per call
        got = planes_np(sup)
        assert got[0].shape == (A, S * (S - 1) // 2)
        assert np.array_equal(got[0], want_sum) and np.array_equal(got[1], want_cnt) and got[2] == want_counters, (A, S, m, chunk)
        if first is None:
            first = sup.state.clone()
        else:
            assert torch.equal(sup.state, first)                         # the whole state, header and padding included
    # a shuffled order of the same chunks with an int32 skip mask
    sup = SW.SubsetPairSupport(A, S, m, device="cuda")
    starts = list(range(0, n, 4099))
    for g0 in rng.permutation(starts):
        sup.update(vd[g0:g0 + 4099], int(g0), sd[g0:g0 + 4099].to(torch.int32))
    assert torch.equal(sup.state, first)
    # the exact identities against the per-locus planes, filled on the device from the same stream: no twin involved
    loci = SW.SubsetSupport(A, S, m, device="cuda")
    loci.update(vd, 0, sd)
    l_sum, l_cnt, l_counters = planes_np(loci)
    got_sum, got_cnt, got_counters = planes_np(sup)
    assert got_counters == l_counters and l_counters[1] >= 2
    assert np.array_equal(PS.unpack(S, got_sum).sum(axis=2), (m - 1) * l_sum) and np.array_equal(PS.unpack(S, got_cnt).sum(axis=2), (m - 1) * l_cnt)
    live = ~skip & (v >= 0) & (v <= 1)
    q = np.asarray([SR.quantum(x) if ok else 0 for x, ok in zip(v, live)], dtype=np.int64)
    pairs = m * (m - 1) // 2
    assert np.array_equal(got_cnt.sum(axis=1), pairs * live.reshape(A, cm).sum(axis=1))
    assert np.array_equal(got_sum.sum(axis=1), pairs * q.reshape(A, cm).sum(axis=1))
    # without a skip mask every row is accepted or rejected; a larger vmax accepts more
    sup = SW.SubsetPairSupport(A, S, m, vmax=2.0, device="cuda")
    sup.update(vd, 0)
    w = PS.pair_support(A, S, m, v, None, 0, vmax=2.0)
    got = planes_np(sup)
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2] and got[2][0] + got[2][1] == n


def test_pair_refusals_on_the_device():
    sup = SW.SubsetPairSupport(4, 9, 3, device="cuda")
    v = torch.zeros(10, device="cuda")
    with _lib.launch_log() as log:
        with pytest.raises(_lib.MatchaHipError, match="outside"):
            sup.update(v, 4 * 84 - 9)
        with pytest.raises(_lib.MatchaHipError, match="outside"):
            sup.update(v, -1)
        with pytest.raises(ValueError):
            sup.update(v.double(), 0)
        with pytest.raises(ValueError):
            sup.update(v, 0, torch.zeros(9, device="cuda"))
        sup.update(v[:0], 0)                                             # nothing to do: nothing launched
        for bad in ((0, 9, 3), (4, 1, 3), (4, 33, 3), (4, 9, 1), (4, 9, 0), (4, 9, 9)):
            with pytest.raises(ValueError):
                SW.SubsetPairSupport(*bad, device="cuda")
        for vmax in (0.0, float("nan"), float(1 << 21)):
            with pytest.raises(ValueError):
                SW.SubsetPairSupport(4, 9, 3, vmax=vmax, device="cuda")
    assert not log.counts
    total, cnt, counters = planes_np(sup)
    assert total.shape == (4, 36) and not total.any() and not cnt.any() and counters == [0, 0]
    assert not sup.state.any()
    i, j = SW.SubsetPairSupport.pair_index(9, "cuda")
    assert i.is_cuda and torch.equal(torch.stack([i, j]).cpu(), torch.triu_indices(9, 9, 1))


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_pair_sweep_against_reference_logits(mode):
    g = gold("g16_subsets_tiny.npz")
    clf = load_tiny(mode)
    for i in PAIR_CASES:
        clusters, m, comp, gap, W = g16_case(g, i)
        kw = dict(mode="drop" if comp else "keep", min_gap=gap, top=8, width=W)
        A, S_max = len(clusters), max(len(c) for c in clusters)
        with _lib.launch_log() as log:
            out = SW.decomposition_sweep(clf, clusters, m, pair_support=True, **kw)
        n_sizes = len(set(len(c) for c in clusters))
        assert log.counts[PAIR] == log.counts[SUPPORT] == n_sizes        # one pair update per support update
        assert log.counts["subset_pair_init_kernel"] == n_sizes == log.counts["subset_pair_read_kernel"]
        plain = SW.decomposition_sweep(clf, clusters, m, **kw)
        keys = OLD_KEYS + (DROP_ONLY if comp else ())
        assert set(out) - set(plain) == set(PAIR_KEYS) and set(plain) <= set(out)
        assert all(torch.equal(out[key], plain[key]) for key in keys)    # every earlier key, bit for bit
        assert all(out[key] == plain[key] for key in ("n_candidates", "n_invalid", "n_excluded"))
        assert out["pair_sum"].shape == out["pair_count"].shape == out["pair_mean"].shape == (A, S_max, S_max)
        assert out["pair_sum"].dtype == torch.float64 and out["pair_count"].dtype == torch.long and out["pair_mean"].dtype == torch.float32
        got_sum, got_cnt = out["pair_sum"].cpu().numpy(), out["pair_count"].cpu().numpy()
        for a, (s, _, valid, _, want_cnt, want) in enumerate(g16_pair_reference(g, mode, i)):
            assert s == len(clusters[a])
            assert np.array_equal(got_cnt[a, :s, :s], want_cnt)          # the valid ranks' choices, exactly
            rel = float(np.abs(got_sum[a, :s, :s] - want).max() / np.abs(want).max())
            print(f"{mode} case {i} cluster {a}: pair_sum rel {rel:.2e}")
            assert rel <= TOL, (mode, i, a, rel)
            assert not got_sum[a, s:].any() and not got_sum[a, :, s:].any() and not got_cnt[a, s:].any() and not got_cnt[a, :, s:].any()
        for key in PAIR_KEYS:
            assert torch.equal(out[key], out[key].transpose(1, 2)) and not torch.diagonal(out[key], dim1=1, dim2=2).any(), key
        hit = out["pair_count"] > 0
        assert torch.equal(out["pair_mean"][hit], (out["pair_sum"][hit] / out["pair_count"][hit]).float()) and not out["pair_mean"][~hit].any()
        for chunk_rows in (37, 4099):                                    # the cut is not part of the result
            again = SW.decomposition_sweep(clf, clusters, m, pair_support=True, chunk_rows=chunk_rows, **kw)
            assert all(torch.equal(again[key], out[key]) for key in keys + PAIR_KEYS), (mode, i, chunk_rows)
    clusters, m, comp, gap, W = g16_case(g, 3)                           # drop one locus: no pair
    assert m == 1
    with _lib.launch_log() as log:
        with pytest.raises(ValueError, match="pair_support"):
            SW.decomposition_sweep(clf, clusters, m, mode="drop", min_gap=gap, top=8, width=W, pair_support=True)
    assert not log.counts


def test_defaults_unchanged_and_pairs_without_support():
    clf = load_tiny("table")
    rng = np.random.default_rng(12)
    clusters = [sorted(int(v) for v in rng.choice(np.arange(1, 65), size=s, replace=False)) for s in (9, 2, 12, 9, 3)]
    with _lib.launch_log() as log:
        out = SW.decomposition_sweep(clf, clusters, 3, top=5)
    assert not PAIR_KERNELS & set(log.counts) and not set(PAIR_KEYS) & set(out) and log.counts[SUPPORT] == 3
    with _lib.launch_log() as log:
        bare = SW.decomposition_sweep(clf, clusters, 3, top=5, support=False, pair_support=True)
    assert SUPPORT not in log.counts and log.counts[PAIR] == 3 and not any(key.startswith("support") for key in bare)
    both = SW.decomposition_sweep(clf, clusters, 3, top=5, pair_support=True)
    assert all(torch.equal(bare[key], both[key]) for key in PAIR_KEYS + ("rows", "logit", "rank", "count"))
    assert all(torch.equal(out[key], both[key]) for key in OLD_KEYS)
    assert not both["pair_count"][1].any() and not both["pair_sum"][1].any()                 # two loci, three wanted: not swept
    assert bool((both["pair_count"][0, :9, :9] == 7 * (1 - torch.eye(9, dtype=torch.long, device="cuda"))).all())    # C(7, 1) triples through a pair
    assert bool((both["pair_count"][4, :3, :3].sum() == 6)) and not both["pair_count"][4, 3:].any()
    # every choice of a cluster contains each of its positions m / s of the time: the pair planes sum to (m - 1) x the locus planes
    assert torch.equal(both["pair_count"].sum(dim=2), 2 * both["support_count"])
    empty = SW.decomposition_sweep(clf, [[5, 9], [7]], 3, pair_support=True)
    assert all(empty[key].shape == (2, 2, 2) and not empty[key].any() for key in PAIR_KEYS)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_decompose_pair_support(tmp_path):
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
            f.write("\t".join("%s:%d" % (node2bin[int(v)].split(":")[0], int(node2bin[int(v)].split(":")[1]) + R.FIXTURE_RES // 3)
                              for v in rng.permutation(ids)) + "\n")
    clf = load_tiny("table")
    out = os.path.join(tmp_path, "decompose.tsv")
    ppath = os.path.join(tmp_path, "decompose_pairs.npz")
    PR.main(["decompose", "-i", ipath, "--size", "3", "--top", "6", "-o", out, "--config", cpath])
    assert not os.path.exists(ppath)                                     # without the flag: what it wrote before
    with np.load(os.path.join(tmp_path, "decompose.npz")) as f:
        before = {key: f[key] for key in f.files}
    assert set(before) == {"clusters", *OLD_KEYS}
    for size, extra in ((3, ()), (2, ("--drop",))):
        PR.main(["decompose", "-i", ipath, "--size", str(size), "--top", "6", "-o", out, "--config", cpath, "--pair-support", *extra])
        with np.load(ppath) as f:
            z = {key: f[key] for key in f.files}
        assert set(z) == {"sizes", "offsets", "pair_mean", "pair_count"}
        assert z["sizes"].tolist() == [2, 9, 25] and z["offsets"].tolist() == [0, 4, 85, 710] and z["sizes"].dtype == z["offsets"].dtype == np.int64
        assert z["pair_mean"].shape == z["pair_count"].shape == (710,) and z["pair_mean"].dtype == np.float32 and z["pair_count"].dtype == np.int64
        ref = SW.decomposition_sweep(clf, clusters, size, mode="drop" if extra else "keep", top=6, pair_support=True)
        for a, s in enumerate((2, 9, 25)):
            lo, hi = z["offsets"][a], z["offsets"][a + 1]
            mean, cnt = z["pair_mean"][lo:hi].reshape(s, s), z["pair_count"][lo:hi].reshape(s, s)
            assert np.array_equal(mean, mean.T) and np.array_equal(cnt, cnt.T) and not np.diag(cnt).any()
            assert np.array_equal(mean, ref["pair_mean"][a, :s, :s].cpu().numpy()) and np.array_equal(cnt, ref["pair_count"][a, :s, :s].cpu().numpy())
        assert not z["pair_count"][:4].any() and z["pair_count"][4:85].sum() > 0          # two loci: no triple, and nothing left without two
        with np.load(os.path.join(tmp_path, "decompose.npz")) as f:
            assert set(f.files) == {"clusters", *OLD_KEYS} | (set(DROP_ONLY) if extra else set())
            if not extra:
                assert all(np.array_equal(f[key], before[key]) for key in before)
    os.remove(ppath)
    with pytest.raises(ValueError, match="pair-support"):
        PR.main(["decompose", "-i", ipath, "--size", "1", "--drop", "--top", "6", "-o", out, "--config", cpath, "--pair-support"])
    assert not os.path.exists(ppath)
