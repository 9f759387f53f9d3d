"""The distance-matched expectation on the MI355X (csrc/expected.hip, matcha_amd/expected.py): strata, planes and
enrichment bit for bit against the numpy restatement (tests/expected_ref.py) for any row order and any cutting of the stream, on the
block-level (LDS) and on the direct path; kway_expected, kway_enriched_sweep and kway_map(expected=...) on the reference's two tiny
models and against the reference's own logits (g11); the CLI."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd import expected as EX
from matcha_amd import predict as PR
from matcha_amd import sweep as SW
from matcha_amd.sampler import HyperedgeSet
from tests import denoise_ref as R
from tests import expected_ref as XR
from tests.helpers import GOLD, gold
from tests.pairmap_ref import pairmap_ref
from tests.test_cpu_expected import EDGES, MIN_COUNT, TOL, g11_reference
from tests.test_cpu_kway import brute
from tests.test_hip_kway import load_tiny
from tests.test_hip_pairmap import SPECIALS, g11_case

pytestmark = pytest.mark.gpu

E15 = (2, 3, 5, 8, 9, 13, 16, 21, 32, 34, 55, 64, 89, 128, 144)
EDGE_SETS = ((), (2,), EDGES, E15)
SIZES = (1, 63, 64, 65, 257, 4099)
PLANES = ("count", "sum", "sumsq")


def make_rows(n, L, k, edges, seed, ordered=False):
    """n rows of width L: ascending k-tuples whose gaps sit exactly on, one below and one above every edge (and at 1 and far out), zero-padded;
    about a fifth of them spoiled -- descending, a repeated id, a hole, one id too many or too few -- and some ids replaced by 2^40 (valid as
    a last id: a gap beyond every edge; invalid anywhere else)."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[1, 2, 3, 1000], np.asarray(edges, dtype=np.int64), np.asarray(edges, dtype=np.int64) - 1,
                                     np.asarray(edges, dtype=np.int64) + 1]))
    pool = pool[pool >= 1]
    x = np.zeros((n, L), dtype=np.int64)
    x[:, 0] = rng.integers(1, 40, n)
    for c in range(1, k):
        x[:, c] = x[:, c - 1] + rng.choice(pool, n)
    kind = rng.integers(0, 25, n)
    for i in np.flatnonzero(kind < 6):
        if kind[i] == 0:                                                 # descending somewhere
            c = rng.integers(0, k - 1)
            x[i, c], x[i, c + 1] = x[i, c + 1], x[i, c]
        elif kind[i] == 1:                                               # a repeated id
            c = rng.integers(0, k - 1)
            x[i, c + 1] = x[i, c]
        elif kind[i] == 2 and k < L:                                     # a hole: a zero, then an id
            x[i, rng.integers(k, L)] = x[i, k - 1] + 7
            if x[i, k] != 0 and k + 1 < L and x[i, k + 1] == 0:
                x[i, k], x[i, k + 1] = 0, x[i, k]
        elif kind[i] == 3 and k < L:                                     # one id too many
            x[i, k] = x[i, k - 1] + 3
        elif kind[i] == 4:                                               # one id too few (none at all for some)
            x[i, rng.integers(0, k):] = 0
        else:
            x[i, rng.integers(0, k)] = 1 << 40
    if ordered:
        x = x[np.lexsort(x.T[::-1])]
    return x


def case_values(n, seed, scale=1.0):
    """values in [0, scale] salted with SPECIALS (each in a kept and in a skipped row where n allows) and a random skip mask."""
    rng = np.random.default_rng(seed)
    v = (rng.random(n) * scale).astype(np.float32)
    skip = ((rng.random(n) < 0.15) * rng.integers(1, 5, n)).astype(np.int32)
    where = rng.permutation(n)[:2 * len(SPECIALS)]
    v[where] = np.asarray(SPECIALS + SPECIALS, dtype=np.float32)[:len(where)]
    skip[where] = np.repeat([0, 2], len(SPECIALS))[:len(where)]
    return v, skip


def run_stats(x, v, skip, k, edges, planes="all", pieces=None, vmax=1.0, shift=32, direct=False):
    st = EX.GapStats(EX.GapStrata(k, edges), planes, vmax=vmax, shift=shift, direct=direct)
    xt, vt = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(v.copy()).cuda()       # the shared cases are read-only
    kt = None if skip is None else torch.from_numpy(skip.copy()).cuda()
    piece = len(x) if pieces is None else pieces
    for a in range(0, len(x), piece):
        st.update(xt[a:a + piece], vt[a:a + piece], None if kt is None else kt[a:a + piece])
    return {key: t.cpu().numpy() for key, t in st.read().items()}


def assert_same(got, ref, names=PLANES):
    assert set(got) == set(names) | {"counters"}
    for name in names:
        a, b = got[name], ref[name]
        assert a.shape == b.shape and a.dtype == b.dtype == np.int64, name
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    assert got["counters"].tolist() == [ref["n_rows"], ref["n_rejected"]]


# ---- 1. strata -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 5, 8])
def test_strata_ids_bitwise_equal_to_the_restatement(L):
    seed = 100 * L
    seen_valid = seen_invalid = 0
    for edges in EDGE_SETS:
        for k in range(2, L + 1):
            if (len(edges) + 1) ** (k - 1) > 1 << 20:
                with pytest.raises(ValueError, match="2\\^20"):
                    EX.GapStrata(k, edges)
                continue
            st = EX.GapStrata(k, edges)
            seed += 1
            full = make_rows(SIZES[-1], L, k, edges, seed)
            ref = XR.strata_ref(full, k, edges)
            for n in SIZES:
                with _lib.launch_log() as log:
                    got = st.ids(torch.from_numpy(full[:n]).cuda())
                assert log.counts == {"gap_enrich_kernel": 1}
                got = got.cpu().numpy()
                assert got.dtype == np.int32 and np.array_equal(got, ref[:n]), (L, k, edges, n, int((got != ref[:n]).sum()))
            assert ref.max() < st.n_strata
            seen_valid += int((ref >= 0).sum())
            seen_invalid += int((ref < 0).sum())
            if len(edges) >= 1 and k >= 3:
                assert len(np.unique(ref)) > min(st.n_strata, 30) // 2   # the rows spread over the strata
    assert seen_valid > 2 * seen_invalid > 0


def test_strata_on_and_below_every_edge_and_invalid_rows():
    for edges in (EDGES, E15):
        st = EX.GapStrata(2, edges)
        x = np.asarray([[7, 7 + e + d] for e in edges for d in (-1, 0)], dtype=np.int64)
        got = st.ids(torch.from_numpy(x).cuda()).cpu().numpy()
        assert got.tolist() == [c for j in range(len(edges)) for c in (j, j + 1)]
    st = EX.GapStrata(3, EDGES)
    bad = np.asarray([[9, 5, 12, 0, 0], [5, 5, 12, 0, 0], [5, 9, 9, 0, 0], [5, 0, 9, 12, 0], [5, 9, 0, 0, 12], [5, 9, 0, 0, 0], [5, 9, 12, 13, 0],
                      [0, 0, 0, 0, 0], [0, 5, 9, 12, 0], [-4, 5, 9, 0, 0], [1 << 40, 5, 9, 0, 0], [5, 1 << 40, 9, 0, 0]], dtype=np.int64)
    good = np.asarray([[5, 9, 1 << 40, 0, 0], [5, 6, 7, 0, 0], [1, 9, 11, 0, 0], [(1 << 40) - 1, 1 << 40, (1 << 40) + 8, 0, 0]], dtype=np.int64)
    got = st.ids(torch.from_numpy(np.concatenate([bad, good])).cuda()).cpu().numpy()
    assert got.tolist() == [-1] * len(bad) + [2 * 4 + 3, 0, 3 * 4 + 1, 0 * 4 + 3]
    assert np.array_equal(got, XR.strata_ref(np.concatenate([bad, good]), 3, EDGES))
    with pytest.raises(ValueError):
        st.ids(torch.zeros(4, 2, dtype=torch.long, device="cuda"))      # narrower than k
    with pytest.raises(ValueError):
        st.ids(torch.zeros(4, 9, dtype=torch.long, device="cuda"))


# ---- 2. planes -----------------------------------------------------------------------------------------------------------------------
# (k, L, edges, the update kernel the launch log must name): 16 strata accumulate in LDS; 65 536 strata x 3 planes x 8 B = 1.5 MiB cannot
PATHS = {"lds": (3, 3, EDGES, "gap_stats_update_kernel"), "lds_wide": (3, 8, E15, "gap_stats_update_kernel"),
         "direct": (5, 5, E15, "gap_stats_update_direct_kernel")}


@pytest.fixture(scope="module")
def plane_cases():
    """Per path: ordered and shuffled rows of 4 099, their values and skips, and the restatement's planes -- computed once, read-only."""
    out = {}
    for name, (k, L, edges, kernel) in PATHS.items():
        for ordered in (True, False):
            x = make_rows(4099, L, k, edges, 7 + len(name), ordered)
            v, skip = case_values(4099, 11 + ordered)
            ref = XR.stats_ref(x, v, k, edges, skip=skip)
            for a in (x, v, skip, ref["count"], ref["sum"], ref["sumsq"]):
                a.setflags(write=False)
            out[(name, ordered)] = (x, v, skip, ref)
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
def test_planes_bitwise_equal_to_the_restatement_ordered_shuffled_and_cut(path, plane_cases):
    k, L, edges, kernel = PATHS[path]
    for ordered in (True, False):
        x, v, skip, ref = plane_cases[(path, ordered)]
        assert ref["n_rejected"] >= 4 and ref["count"].max() > 1 and ref["n_rows"] > 2000
        for piece in (None, 1, 37, 64):
            if piece == 1 and not ordered:
                continue
            with _lib.launch_log() as log:
                got = run_stats(x, v, skip, k, edges, pieces=piece)
            n_updates = 1 if piece is None else -(-len(x) // piece)
            assert log.counts == {"gap_stats_init_kernel": 1, kernel: n_updates, "gap_stats_read_kernel": 1}
            assert_same(got, ref)
        for n in SIZES[:-1]:                                             # short streams: one lane, one wavefront and a lane, a block and a lane
            assert_same(run_stats(x[:n], v[:n], skip[:n], k, edges), XR.stats_ref(x[:n], v[:n], k, edges, skip=skip[:n]))
        assert_same(run_stats(x, v, None, k, edges), XR.stats_ref(x, v, k, edges))
    # the two paths hold the same planes: the A/B switch of the block-level accumulation
    with _lib.launch_log() as log:
        got = run_stats(x, v, skip, k, edges, direct=True)
    assert log.counts["gap_stats_update_direct_kernel"] == 1 and "gap_stats_update_kernel" not in log.counts
    assert_same(got, ref)


@pytest.mark.parametrize("planes", [1, 2, 3, 4, 5, 6, 7, ["sum"], ["count", "sumsq"]])
def test_plane_masks(planes, plane_cases):
    names = [p for p in PLANES if _lib.GAP_PLANES[p] & planes] if isinstance(planes, int) else [p for p in PLANES if p in planes]
    for path in ("lds", "direct"):
        k, L, edges, kernel = PATHS[path]
        x, v, skip, ref = plane_cases[(path, True)]
        with _lib.launch_log() as log:
            got = run_stats(x, v, skip, k, edges, planes=planes)
        # one plane of 65 536 strata (512 KiB) still exceeds the LDS budget
        assert log.counts == {"gap_stats_init_kernel": 1, kernel: 1, "gap_stats_read_kernel": 1}
        assert_same(got, ref, names)


def test_one_stratum_takes_everything_and_the_largest_lds_table():
    st = EX.GapStrata(3, EDGES)
    x = np.tile(np.asarray([[3, 5, 40]], dtype=np.int64), (100000, 1))
    with _lib.launch_log() as log:
        got = run_stats(x, np.ones(100000, dtype=np.float32), None, 3, EDGES)
    assert log.counts["gap_stats_update_kernel"] == 1
    s = 1 * 4 + 3
    assert got["count"][s] == 100000 and got["sum"][s] == got["sumsq"][s] == 100000 << 32 and got["count"].sum() == 100000
    assert got["counters"].tolist() == [100000, 0]
    # 4 096 strata x 2 planes x 8 B = 64 KiB: exactly the budget, still in LDS; with the third plane direct
    for planes, kernel in ((3, "gap_stats_update_kernel"), (7, "gap_stats_update_direct_kernel")):
        xs = make_rows(4099, 4, 4, E15, 5, True)
        v, skip = case_values(4099, 6)
        with _lib.launch_log() as log:
            got = run_stats(xs, v, skip, 4, E15, planes=planes)
        assert log.counts[kernel] == 1
        assert_same(got, XR.stats_ref(xs, v, 4, E15, skip=skip), [p for p in PLANES if _lib.GAP_PLANES[p] & planes])


# ---- 3. shift and vmax ---------------------------------------------------------------------------------------------------------------
def test_shift_and_vmax_are_part_of_the_contract(plane_cases):
    k, L, edges, _ = PATHS["lds"]
    x, v, skip, _ = plane_cases[("lds", True)]
    x, skip = x[:257], skip[:257]
    v = (v[:257] * np.float32(3.0)).astype(np.float32)                   # values up to 3, 1.5 * 3 = 4.5 among them
    for shift in (16, 24, 32):
        for vmax in (1.0, 4.5, float(2 ** 20)):
            fits = vmax * vmax * 2.0 ** shift <= 2.0 ** 62               # one row's squared term
            names = PLANES if fits else PLANES[:2]
            ref = XR.stats_ref(x, v, k, edges, vmax=vmax, shift=shift, skip=skip)
            assert_same(run_stats(x, v, skip, k, edges, planes=list(names), vmax=vmax, shift=shift), ref, names)
            if not fits:
                with pytest.raises(ValueError, match="smaller shift"):
                    EX.GapStats(EX.GapStrata(k, edges), "all", vmax=vmax, shift=shift)
    rows = np.tile(np.asarray([[3, 4, 5]], dtype=np.int64), (64, 1))
    got = run_stats(rows, np.full(64, 2.0 ** 20, dtype=np.float32), None, k, edges, vmax=float(2 ** 20), shift=16)
    assert got["sum"][0] == 64 << 36 and got["sumsq"][0] == 64 << 56 and got["count"][0] == 64 and got["counters"].tolist() == [64, 0]
    res = EX.stats_result(got, float(2 ** 20), 16)
    assert res["mean"][0] == 2.0 ** 20 and res["var"][0] == 0.0


# ---- 4. enrichment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,k,edges", [(3, 3, EDGES), (5, 4, (2,)), (8, 5, E15), (2, 2, ())])
def test_enrich_bitwise_equal_to_numpy_float32(L, k, edges):
    st = EX.GapStrata(k, edges)
    rng = np.random.default_rng(L)
    offset = rng.normal(size=st.n_strata).astype(np.float32)
    scale = (rng.random(st.n_strata) * 3 + 0.1).astype(np.float32)
    salt = rng.permutation(st.n_strata)
    for j, val in enumerate((np.nan, np.inf, -np.inf, 0.0)):
        if j < st.n_strata:
            offset[salt[j]] = val
    for n in SIZES:
        x = make_rows(n, L, k, edges, 50 + n)
        score = (rng.normal(size=n) * 4).astype(np.float32)
        score[rng.permutation(n)[:4]] = np.asarray([-0.0, 0.0, np.inf, np.nan], dtype=np.float32)[:min(n, 4)]
        s = XR.strata_ref(x, k, edges)
        ref = XR.enrich_ref(score, s, offset, scale)
        with _lib.launch_log() as log:
            got, got_s = st.enrich(torch.from_numpy(x).cuda(), torch.from_numpy(score).cuda(), torch.from_numpy(offset).cuda(),
                                   torch.from_numpy(scale).cuda(), want_strata=True)
        assert log.counts == {"gap_enrich_kernel": 1}
        got, got_s = got.cpu().numpy(), got_s.cpu().numpy()
        assert np.array_equal(got_s, s) and got.dtype == np.float32
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32)), (n, L)
        assert nan[s < 0].all()
        only = st.enrich(torch.from_numpy(x).cuda(), torch.from_numpy(score).cuda(), torch.from_numpy(offset).cuda(), torch.from_numpy(scale).cuda())
        assert np.array_equal(only.cpu().numpy().view(np.uint32)[~nan], got.view(np.uint32)[~nan])
    # a product that FMA contraction would round differently: (a - b) * c with a - b inexact
    one = EX.GapStrata(2, ())
    a = np.asarray([1.0 + 2.0 ** -23, 3.1415927, 1e-3], dtype=np.float32)
    off, sc = np.asarray([2.0 ** -24 * 3], dtype=np.float32), np.asarray([1.0 / 3.0], dtype=np.float32)
    got = one.enrich(torch.tensor([[1, 2]] * 3, device="cuda"), torch.from_numpy(a).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(sc).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ((a - off[0]).astype(np.float32) * sc[0]).astype(np.float32).view(np.uint32))
    with pytest.raises(ValueError):
        one.enrich(torch.tensor([[1, 2]], device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda"))


# ---- 5. kway_expected ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """Per model: the reference's tiny classifier, and per g11 case its region, the candidates and the device's own logits and
    probabilities of them (one forward over all rows on the sweep's kernel route)."""
    g = gold("g11_kway_tiny.npz")
    out = {"N": int(np.sum(g["num"]))}
    for mode in ("table", "adj"):
        clf = load_tiny(mode)
        clf.eval()
        cases = []
        for i in range(3):
            lo, hi, k, gap = g11_case(g, i)
            rows = g[f"rows_c{i}"]
            with torch.no_grad(), _lib.option("disable_small_batch"):
                logit = clf(torch.from_numpy(rows).cuda()).reshape(-1)
                value = torch.sigmoid(logit).cpu().numpy()
            cases.append(dict(lo=lo, hi=hi, k=k, gap=gap, rows=rows, logit=logit.cpu().numpy(), value=value))
        out[mode] = (clf, cases)
    return out


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_kway_expected_is_the_restatement_of_the_device_probabilities(mode, tiny):
    clf, cases = tiny[mode]
    for c in cases:
        lo, hi, k, gap, rows = c["lo"], c["hi"], c["k"], c["gap"], c["rows"]
        ref = XR.stats_ref(rows, c["value"], k, EDGES)
        mean, var = XR.moments_ref(ref)
        n_chunks = {37: -(-len(rows) // 37), 4099: 1, 1 << 20: 1}
        for chunk_rows in (37, 4099, 1 << 20):
            with _lib.launch_log() as log:
                ex = EX.kway_expected(clf, [(lo, hi)], k, gap, edges=EDGES, chunk_rows=chunk_rows)
            assert log.counts["gap_stats_update_kernel"] == log.counts["kway_rows_kernel"] == n_chunks[chunk_rows]
            assert log.counts["gap_stats_init_kernel"] == log.counts["gap_stats_read_kernel"] == 1
            assert all(np.array_equal(ex.raw[name], ref[name]) for name in PLANES), (mode, chunk_rows)
            assert np.array_equal(ex.count, ref["count"]) and np.array_equal(ex.mean, mean) and np.array_equal(ex.var, var)
            assert (ex.n_rows, ex.n_rejected) == (len(rows), 0) and ex.regions == ((lo, hi),) and (ex.k, ex.min_gap, ex.width) == (k, gap, k)
        assert clf.check_ids                                             # the per-call check is back on
    # two regions in one call: the integer sum of the two single-region calls (k = 3 candidates of the regions of cases 0 and 2)
    (a, b) = ((cases[0]["lo"], cases[0]["hi"]), (cases[2]["lo"], cases[2]["hi"]))
    both = EX.kway_expected(clf, [a, b], 3, 2, edges=EDGES, chunk_rows=100)
    one, two = (EX.kway_expected(clf, [r], 3, 2, edges=EDGES) for r in (a, b))
    assert all(np.array_equal(both.raw[name], one.raw[name] + two.raw[name]) for name in PLANES)
    assert both.n_rows == one.n_rows + two.n_rows == len(brute(a[0], a[1] - a[0], 3, 2)) + len(brute(b[0], b[1] - b[0], 3, 2))
    assert two.n_rows > 0 and both.regions == (a, b)
    default = EX.kway_expected(clf, [a], 3, 2)                           # default edges: the powers of two below the region's length
    assert default.edges == EX.default_gap_edges(a[1] - a[0], 3) and default.count.sum() == one.n_rows
    with pytest.raises(IndexError):
        EX.kway_expected(clf, [(tiny["N"] - 10, tiny["N"] + 10)], 3, 1)  # a region beyond the model's tables: raised once, at the end
    with pytest.raises(ValueError, match="vmax"):
        EX.kway_expected(clf, [a], 3, 2, task_mode="regress")


# ---- 6. kway_enriched_sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_enriched_sweep_against_reference_logits(mode, tiny):
    """The top-K set of the reference's own logits (K where its sorted enrichment has its largest gap, >= 10 tol: tests/test_cpu_expected.py)
    and the enrichment within tol.  Measured on the MI355X: largest |enrich - reference| / tol 0.0029 (table), 0.0017 (adj)."""
    clf, cases = tiny[mode]
    for i, c in enumerate(cases):
        K, gap, tol, ref_enrich, ref_strata, ref_count, ref_offset = g11_reference(i, mode)
        order = np.argsort(-np.where(np.isnan(ref_enrich), -np.inf, ref_enrich.astype(np.float64)), kind="stable")[:K]
        out = EX.kway_enriched_sweep(clf, c["lo"], c["hi"], c["k"], c["gap"], top=K, edges=EDGES, min_count=MIN_COUNT, mode="logodds")
        rank, enrich = out["rank"].cpu().numpy(), out["enrich"].cpu().numpy()
        err = np.abs(enrich.astype(np.float64) - ref_enrich[rank].astype(np.float64))
        print(f"{mode} case {i}: K={K} gap={gap:.4g} tol={tol:.4g} max error / tol {err.max() / tol:.3g}")
        assert len(rank) == K and set(rank.tolist()) == set(order.tolist()), (mode, i)
        assert (err <= tol).all(), (mode, i, err.max(), tol)
        assert np.array_equal(out["rows"].cpu().numpy(), c["rows"][rank]) and np.array_equal(out["stratum"].cpu().numpy(), ref_strata[rank])
        assert out["n_candidates"] == len(c["rows"]) and out["n_excluded"] == 0
        assert out["n_undersampled"] == int(np.isnan(ref_enrich).sum()) == (0, 0, 4)[i]
        assert np.array_equal(out["expected_table"].count, ref_count)
        assert (np.diff(enrich) <= 0).all() and np.array_equal(out["expected"].cpu().numpy(), out["expected_table"].mean[ref_strata[rank]])


def test_enriched_sweep_ties_to_sweep_exclusion_cache_width_and_regress(tiny):
    clf, cases = tiny["table"]
    c = cases[0]
    lo, hi, k, gap, rows = c["lo"], c["hi"], c["k"], c["gap"], c["rows"]
    n = len(rows)
    # one stratum: the enrichment is the logit minus one constant -- kway_sweep's ranks in kway_sweep's order
    plain = SW.kway_sweep(clf, lo, hi, k, gap, top=50)
    single = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=50, edges=[], mode="logodds")
    assert torch.equal(single["rank"], plain["rank"]) and torch.equal(single["logit"], plain["logit"]) and torch.equal(single["rows"], plain["rows"])
    assert single["expected_table"].count.tolist() == [n] and not single["stratum"].any() and single["n_undersampled"] == 0
    # the device's own values through the restatement: the whole ranking, bit for bit
    full = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=n, edges=EDGES, min_count=MIN_COUNT)
    ref = XR.stats_ref(rows, c["value"], k, EDGES)
    mean, var = XR.moments_ref(ref)
    offset, scale = XR.table_ref(ref["count"], mean, var, "logodds", MIN_COUNT)
    want = XR.enrich_ref(c["logit"], XR.strata_ref(rows, k, EDGES), offset, scale)
    rank = full["rank"].cpu().numpy()
    assert len(rank) == n and np.array_equal(full["enrich"].cpu().numpy().view(np.uint32), want[rank].view(np.uint32))
    assert np.array_equal(full["logit"].cpu().numpy().view(np.uint32), c["logit"][rank].view(np.uint32))
    assert np.array_equal(rank, np.lexsort((np.arange(n), -want.astype(np.float64))))          # higher enrichment first, then lower rank
    # undersampled: min_count above every count gives an empty result
    with _lib.launch_log() as log:
        none = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=10, edges=EDGES, min_count=10 ** 6)
    assert none["n_undersampled"] == none["n_candidates"] == n and all(len(none[key]) == 0 for key in ("rows", "logit", "proba", "rank", "enrich", "stratum", "expected"))
    assert none["rows"].shape == (0, k)
    # known hyperedges: skipped and counted in the ranking, still part of the expectation
    known = rank[:100]
    hset = HyperedgeSet(torch.from_numpy(rows[known]).cuda())
    for chunk_rows in (1 << 20, 37):
        exc = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=n, edges=EDGES, min_count=MIN_COUNT, exclude=hset, chunk_rows=chunk_rows)
        assert exc["n_excluded"] == 100 and exc["n_candidates"] == n and np.array_equal(exc["expected_table"].raw["sum"], ref["sum"])
        assert torch.equal(exc["rank"], full["rank"][100:]) and torch.equal(exc["enrich"], full["enrich"][100:])
    # the cache: the kept logits are the bits a second forward produces
    with _lib.launch_log() as cached_log:
        cached = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=40, edges=EDGES, min_count=MIN_COUNT, chunk_rows=100)
    with _lib.launch_log() as twice_log:
        twice = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=40, edges=EDGES, min_count=MIN_COUNT, chunk_rows=100, cache_rows=0)
    assert all(torch.equal(cached[key], twice[key]) for key in ("rows", "logit", "proba", "rank", "enrich", "stratum", "expected"))
    assert torch.equal(cached["rank"], full["rank"][:40]) and torch.equal(cached["enrich"], full["enrich"][:40])
    assert cached_log.counts["kway_rows_kernel"] == twice_log.counts["kway_rows_kernel"] == 2 * 6 + 1
    assert cached_log.counts["gap_enrich_kernel"] == twice_log.counts["gap_enrich_kernel"] == 6 + 1
    assert sum(cached_log.counts.values()) < sum(twice_log.counts.values())                   # six forwards fewer
    # a given table: the same ranking without the first pass
    with _lib.launch_log() as log:
        given = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=40, expected=full["expected_table"], min_count=MIN_COUNT)
    assert "gap_stats_update_kernel" not in log.counts and torch.equal(given["rank"], cached["rank"]) and torch.equal(given["enrich"], cached["enrich"])
    # a wider batch is another forward (pads are attended), so another expectation; the strata are the same
    wide = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=n, edges=EDGES, min_count=MIN_COUNT, width=5)
    assert wide["rows"].shape == (n, 5) and not wide["rows"][:, 3:].any() and wide["expected_table"].width == 5
    assert np.array_equal(wide["expected_table"].count, ref["count"]) and not np.array_equal(wide["expected_table"].raw["sum"], ref["sum"])
    with torch.no_grad(), _lib.option("disable_small_batch"):
        wl = clf(wide["rows"]).reshape(-1)
    assert torch.equal(wl, wide["logit"])
    # ratio and z on the probabilities; regress: ratio runs, logodds is refused
    for mode in ("ratio", "z"):
        out = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=n, edges=EDGES, min_count=MIN_COUNT, mode=mode)
        o, s = XR.table_ref(ref["count"], mean, var, mode, MIN_COUNT)
        w = XR.enrich_ref(c["value"], XR.strata_ref(rows, k, EDGES), o, s)
        r = out["rank"].cpu().numpy()
        assert np.array_equal(out["enrich"].cpu().numpy().view(np.uint32), w[r].view(np.uint32)) and len(r) == n
    soft = torch.nn.functional.softplus(torch.from_numpy(c["logit"]).cuda()).cpu().numpy()
    reg = EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=n, edges=EDGES, min_count=MIN_COUNT, mode="ratio", task_mode="regress", vmax=64.0)
    sref = XR.stats_ref(rows, soft, k, EDGES, vmax=64.0)
    assert np.array_equal(reg["expected_table"].raw["sum"], sref["sum"]) and reg["expected_table"].task_mode == "regress"
    o, s = XR.table_ref(sref["count"], *XR.moments_ref(sref), "ratio", MIN_COUNT)
    assert np.array_equal(reg["enrich"].cpu().numpy().view(np.uint32), XR.enrich_ref(soft, XR.strata_ref(rows, k, EDGES), o, s)[reg["rank"].cpu().numpy()].view(np.uint32))
    with _lib.launch_log() as log:
        with pytest.raises(ValueError, match="regress"):
            EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=5, edges=EDGES, mode="logodds", task_mode="regress", vmax=64.0)
        with pytest.raises(ValueError, match="vmax"):
            EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=5, edges=EDGES, mode="ratio", task_mode="regress")
        with pytest.raises(ValueError):
            EX.kway_enriched_sweep(clf, lo, hi, k, gap, top=5, mode="median")
        with pytest.raises(ValueError, match="k="):
            EX.kway_enriched_sweep(clf, lo, hi, 4, gap, top=5, expected=full["expected_table"])
        empty = EX.kway_enriched_sweep(clf, lo, lo + 2, 3, 1, top=5)     # two bins, k = 3: no candidates
    assert not log.counts or set(log.counts) <= {"gap_stats_init_kernel", "gap_stats_read_kernel"}
    assert empty["n_candidates"] == 0 and empty["rows"].shape == (0, 3) and empty["n_undersampled"] == 0
    assert clf.check_ids


# ---- 7. the observed-over-expected pair map ------------------------------------------------------------------------------------------
def test_map_with_expected_is_the_pair_map_of_the_device_ratios(tiny):
    clf, cases = tiny["table"]
    names = ("sum", "count", "count_ge", "max")

    def same(out, ref):
        for name in names:
            a, b = out[name].cpu().numpy(), ref[name] / 4294967296.0 if name == "sum" else ref[name]
            assert np.array_equal(a.view(np.uint32) if name == "max" else a, b.view(np.uint32) if name == "max" else b), name

    for i, c in enumerate(cases[:2]):
        lo, hi, k, gap, rows, value = c["lo"], c["hi"], c["k"], c["gap"], c["rows"], c["value"]
        n = hi - lo
        ex = EX.kway_expected(clf, [(lo, hi)], k, gap, edges=EDGES)
        for min_count in (MIN_COUNT, 8):
            offset, scale = ex.table_host("ratio", min_count)
            ratio = XR.enrich_ref(value, XR.strata_ref(rows, k, EDGES), offset, scale)
            for chunk_rows in (1 << 20, 37):
                with _lib.launch_log() as log:
                    out = SW.kway_map(clf, lo, hi, k, gap, expected=ex, min_count=min_count, threshold=1.0, chunk_rows=chunk_rows)
                assert log.counts["gap_enrich_kernel"] == log.counts["pairmap_update_kernel"] == -(-len(rows) // chunk_rows)
                ref = pairmap_ref(rows, ratio, (lo, n), (lo, n), vmax=1024.0, threshold=1.0)
                same(out, ref)
                assert out["n_rejected"] == ref["n_rejected"] == int(np.isnan(ratio).sum()) and out["n_candidates"] == len(rows)
            assert 0 < ref["count_ge"].sum() < ref["count"].sum()        # some candidates above their expectation, some below
        assert int(np.isnan(ratio).sum()) == (0, 30)[i]     # min_count 8 drops 30 of case 1's 715 candidates
        # without expected: what kway_map gave before -- the pair map of the device's probabilities
        plain = SW.kway_map(clf, lo, hi, k, gap)
        same(plain, pairmap_ref(rows, value, (lo, n), (lo, n)))
        assert not torch.equal(plain["sum"], out["sum"])
    with pytest.raises(ValueError, match="ratio"):
        SW.kway_map(clf, lo, hi, k, gap, expected=ex, mode="z")
    with pytest.raises(ValueError, match="k="):
        SW.kway_map(clf, lo, hi, 3, gap, expected=ex)


# ---- 8. CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_kway_and_kmap_enrich(tmp_path):
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
    out, saved = os.path.join(tmp_path, "kway.tsv"), os.path.join(tmp_path, "expected.npz")
    lo, hi = int(cr[2][0]), int(cr[2][1])
    clf = load_tiny("table")

    def run(*extra):
        PR.main(["kway", "--chrom", "2", "--k", "3", "--top", "12", "-o", out, "--config", cpath, *extra])
        return open(out).read()

    plain = run()
    assert all(len(line.split("\t")) == 4 for line in plain.splitlines()) and len(plain.splitlines()) == 12      # what it writes today
    first = run("--enrich", "logodds", "--gap-edges", "2,4,8", "--min-count", "4", "--save-expected", saved)
    ref = EX.kway_enriched_sweep(clf, lo, hi, 3, 2, top=12, edges=EDGES, min_count=4)
    lines = [line.split("\t") for line in first.splitlines()]
    assert len(lines) == 12 and all(len(cols) == 7 for cols in lines)
    rows = ref["rows"].cpu().numpy()
    table = ref["expected_table"]
    for cols, r, p, e, m, s in zip(lines, rows, ref["proba"].cpu().numpy(), ref["enrich"].cpu().numpy(), ref["expected"].cpu().numpy(),
                                   ref["stratum"].cpu().numpy()):
        assert cols[:3] == [node2bin[int(v)] for v in r] and cols[3:6] == [repr(float(p)), repr(float(e)), repr(float(m))]
        assert cols[6] == PR.gap_ranges(table.strata.decode(int(s))) and len(cols[6].split(",")) == 2
    z = np.load(os.path.splitext(out)[0] + ".npz")
    assert np.array_equal(z["enrich"], ref["enrich"].cpu().numpy()) and z["gap_edges"].tolist() == list(EDGES)
    back = EX.GapExpected.load(saved)
    assert np.array_equal(back.count, table.count) and np.array_equal(back.mean, table.mean) and back.regions == ((lo, hi),)
    assert run("--enrich", "logodds", "--min-count", "4", "--load-expected", saved) == first
    every = run("--enrich", "logodds", "--gap-edges", "2,4,8", "--min-count", "4", "--expected-chroms", "all")
    all_ex = EX.kway_expected(clf, [(int(a), int(b)) for a, b in cr], 3, 2, edges=EDGES)
    want = EX.kway_enriched_sweep(clf, lo, hi, 3, 2, top=12, expected=all_ex, min_count=4)
    assert [line.split("\t")[4] for line in every.splitlines()] == [repr(float(e)) for e in want["enrich"].cpu().numpy()]
    assert all_ex.n_rows > table.n_rows and every != first
    # the map form
    mpath = os.path.join(tmp_path, "map.npz")
    PR.main(["kmap", "--chrom", "2", "--k", "3", "-o", mpath, "--config", cpath, "--enrich", "ratio", "--load-expected", saved, "--min-count", "4"])
    z = np.load(mpath)
    want = SW.kway_map(clf, lo, hi, 3, 2, expected=back, min_count=4)
    assert all(np.array_equal(z[name], want[name].cpu().numpy()) for name in ("sum", "mean", "count", "count_ge"))
    assert z["gap_edges"].tolist() == list(EDGES) and np.array_equal(z["expected_count"], back.count)
    with pytest.raises(ValueError, match="gap-edges"):
        run("--enrich", "logodds", "--gap-edges", "4,2")
