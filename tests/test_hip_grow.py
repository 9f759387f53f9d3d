"""Cluster growth on the MI355X (csrc/grow.hip, matcha_amd/sweep.py): the twin table and the twin flags bit for bit against
the set rule of tests/grow_ref.py; one step against the reference's own logits, teacher-forced on its beams (g17); the whole growth bit
for bit against the Python twin fed the device's logits, independent of how it is cut; exclusion, errors and empty cases; the untouched
sweeps; the CLI."""
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
from oracle import hypersagnn as O
from tests import complete_ref as CR
from tests import denoise_ref as R
from tests import grow_ref as GR
from tests.helpers import GOLD, gold, logit_err, oracle_state
from tests.test_cpu_grow import g17_step_arrays, random_beam
from tests.test_cpu_long_rows import golden_oracle
from tests.test_hip_kway import load_tiny
from tests.test_hip_long_rows import LONG, SHORT_ONLY

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the project's tolerance against the reference
ROWS, TWINS, FLAGS = "kway_complete_rows_kernel", "grow_twins_kernel", "grow_twin_flags_kernel"
SEG_KERNELS = {"segtopk_keys_kernel", "segtopk_merge_kernel", "segtopk_commit_kernel"}
KEYS = ("rows", "logit", "proba", "parent", "added", "count", "size", "path")
INTS = ("n_candidates", "n_invalid", "n_twins", "n_excluded", "steps")


def made_beam(rng, B, S, lo, n):
    """int64 [4, B, S].  Seed 0: slot 0 a base row of even ids, then copies with the first, a middle and the last id replaced, an
    identical copy, then copies with one id replaced by a bin of the region (a twin id inside the region; the others lie outside).
    Seed 1: full slots with empty ones between, slots of S - 1 ids, one with a repeated id and one that descends.  Seed 2: as a growth
    makes them (tests/test_cpu_grow.py).  Seed 3: two ids replaced (no relation) and pairs that differ by a shift of the whole row."""
    beam = np.zeros((4, B, S), dtype=np.int64)
    base = 100 + 2 * np.sort(rng.choice(np.arange(60), size=S, replace=False))          # even ids >= 100: odd ones fit between
    swaps = [(0, 51), (S // 2, int(base[S // 2]) + 1), (S - 1, int(base[-1]) + 7), None]
    for j in range(B):
        row = base.copy()
        if j >= 1:
            swap = swaps[j - 1] if j - 1 < len(swaps) else (int(rng.integers(S)), lo + int(rng.integers(n)))
            if swap is not None:
                row[swap[0]] = swap[1]
        beam[0, j] = np.sort(row)
    for j in range(B):
        kind = j % 6
        row = base.copy()
        row[int(rng.integers(S))] += 1                                   # one id off the base: related to the other full slots
        if kind == 1:
            row[:] = 0                                                   # an empty slot between full ones
        elif kind == 2:
            row = np.concatenate([np.sort(row)[:S - 1], [0]])            # a slot of another size (S = 1: empty)
        elif kind == 3 and S >= 2:
            row[1] = row[0]                                              # a repeated id
            row = np.concatenate([row[:2], np.sort(row[2:])])
        elif kind == 4 and S >= 2:
            row = np.sort(row)[::-1]                                     # a slot that descends
        else:
            row = np.sort(row)
        beam[1, j] = row
    beam[2] = random_beam(rng, 1, B, S, lo, n, np.arange(1, 3 * (lo + n)))[0]
    for j in range(B):
        row = base.copy()
        if j % 3 == 1:
            row = base + 2                                               # every id moved: S ids apart, or one when the shift chains
        elif j % 3 == 2 and S >= 2:
            row[0], row[-1] = row[0] - 1, row[-1] + 1                    # two ids replaced
        beam[3, j] = row
    return beam


# ---- the twin table and the flags, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 8, 9, 31])
@pytest.mark.parametrize("B", [1, 2, 5, 64])
def test_twins_grid(B, S):
    rng = np.random.default_rng(1000 * B + S)
    lo, n = 7, 40
    beam = made_beam(rng, B, S, lo, n)
    ref = GR.twin_table(beam)
    with _lib.launch_log() as log:
        twin = SW.grow_twins(torch.from_numpy(beam).cuda())
    assert log.counts == {TWINS: 1}                                      # it, and only it
    got = twin.cpu().numpy()
    assert got.shape == ref.shape == (4 * B, B) and np.array_equal(got, ref), (B, S)
    base = beam[0, 0]
    assert (ref >= lo + n).any() == (B >= 2)                             # twin ids outside the region
    if B >= 5:                                                           # slot 0 against the copies with the first, a middle, the last id replaced
        assert ref[1, 0] == base[0] and ref[2, 0] == base[S // 2] and ref[3, 0] == base[-1] and ref[4, 0] == -1
    if B == 64:
        assert ((ref >= lo) & (ref < lo + n)).any()                      # ... and inside it: two slots with the same id replaced
    # a reused buffer: what lies behind the table is untouched
    buf = torch.full((4 * B * B + 5,), -7, dtype=torch.long, device="cuda")
    again = SW.grow_twins(torch.from_numpy(beam).cuda(), out=buf)
    assert again.data_ptr() == buf.data_ptr() and torch.equal(again, twin) and bool((buf[4 * B * B:] == -7).all())


def test_twins_many_seeds_and_none():
    """Seeds of another shape; more entries than one pass of the grid takes (2^20 blocks of four); A = 0 launches nothing."""
    rng = np.random.default_rng(5)
    beam = np.concatenate([random_beam(rng, 50, 7, 4, 5, 9, np.arange(1, 60)) for _ in range(3)])
    got = SW.grow_twins(torch.from_numpy(beam).cuda()).cpu().numpy()
    assert np.array_equal(got, GR.twin_table(beam)) and (got == -1).any() and (got > 0).any()
    A = (1 << 21) + 3                                                    # two slots of one id: 2^22 + 6 entries
    big = rng.integers(0, 4, size=(A, 2, 1))
    want = np.zeros((2 * A, 2), dtype=np.int64)
    a, b = big[:, 0, 0], big[:, 1, 0]
    want[1::2, 0] = np.where((a == 0) | (b == 0), 0, np.where(a == b, -1, a))
    assert np.array_equal(want[:200], GR.twin_table(big[:100]))
    got = SW.grow_twins(torch.from_numpy(big).cuda())
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    with _lib.launch_log() as log:
        assert SW.grow_twins(torch.zeros(0, 7, 4, dtype=torch.long, device="cuda")).shape == (0, 7)
    assert not log.counts


def test_twin_flags_ranges_and_counts():
    """13 seeds of 5 slots of 3 ids, a region of 70 bins: 4 550 ranks.  Ranges from rank 0, from inside a slot, across a seed boundary
    and up to the last rank; counts around a wavefront and over many blocks; flags that already hold 1; a reused buffer."""
    lo, n, A, B, S = 5, 70, 13, 5, 3
    rng = np.random.default_rng(9)
    beam = random_beam(rng, A, B, S, lo, n, np.arange(1, 200))
    beam[3, 2] = beam[3, 0]                                              # identical slots: every candidate of the later one
    beam[4, 1] = np.sort(np.concatenate([beam[4, 0][:2], [lo + n + 3]]))  # a twin id outside the region: nobody's candidate
    beam[5, 3] = 0                                                       # an empty slot
    beam[6, 1] = beam[6, 1][::-1]                                        # a slot that descends
    tw = GR.twin_flags(beam, lo, n)
    total = A * B * n
    assert tw.shape == (total,) and tw.any() and not tw.all() and tw[(3 * B + 2) * n:(3 * B + 3) * n].all()
    twin = SW.grow_twins(torch.from_numpy(beam).cuda())
    assert np.array_equal(twin.cpu().numpy(), GR.twin_table(beam))
    before = rng.integers(0, 2, size=total).astype(np.int32)
    for count in (1, 63, 64, 65, 4099):
        for rank0 in (0, 3 * n + 41, B * n - 30, total - count):
            buf = torch.full((count + 9,), -7, dtype=torch.int32, device="cuda")
            buf[:count] = torch.from_numpy(before[rank0:rank0 + count]).cuda()
            with _lib.launch_log() as log:
                flag = SW.grow_twin_flags(twin, lo, n, buf, rank0, count)
            assert log.counts == {FLAGS: 1} and flag.data_ptr() == buf.data_ptr()
            want = before[rank0:rank0 + count] | (2 * tw[rank0:rank0 + count].astype(np.int32))
            assert np.array_equal(buf[:count].cpu().numpy(), want), (rank0, count)
            assert bool((buf[count:] == -7).all())                       # memory behind count is untouched
    flag = torch.zeros(total, dtype=torch.int32, device="cuda")
    SW.grow_twin_flags(twin, lo, n, flag)                                # everything, the default
    assert np.array_equal(flag.cpu().numpy(), 2 * tw.astype(np.int32))
    with _lib.launch_log() as log:
        SW.grow_twin_flags(twin, lo, n, flag, total, 0)
        with pytest.raises(IndexError):
            SW.grow_twin_flags(twin, lo, n, flag, total - 1, 2)
    assert not log.counts


# ---- one step against the reference, teacher-forced ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
@pytest.mark.parametrize("case", range(len(GR.G17_CASES)))
def test_grow_step_against_reference_logits(case, mode):
    """Every stored step of the case.  With l the reference's logits of a seed's valid non-twin candidates, theta the B-th largest
    (-inf if there are fewer) and m = 1e-4 max|l|: min(B, #valid) rows are kept, every candidate with l > theta + 2 m among them and
    none with l < theta - 2 m (the threshold and the candidate may each be off by the tolerance)."""
    g = gold("g17_grow_tiny.npz")
    clf = load_tiny(mode)
    (lo, hi), B, gap, sizes, max_size, W = GR.G17_CASES[case]
    n = hi - lo
    for t, active, beam, ref in g17_step_arrays(g, case, mode):
        A_t, B_t, S_t = beam.shape
        seg = B_t * n
        rows, bad, tw = GR.candidates(beam, lo, n, gap, W)
        with _lib.launch_log() as log:
            out = SW.grow_step(clf, beam, lo, hi, beam_out=B, min_gap=gap, width=W)
        ran = {name for name, c in log.counts.items() if c > 0}
        if case == 0:
            assert ran & SHORT_ONLY and not (ran & LONG), sorted(ran)    # width 8: the short forward
        else:
            assert LONG <= ran and not (ran & SHORT_ONLY), sorted(ran)   # widths 12, 16 and 32: the long plan and attention
        assert not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)
        assert log.counts[TWINS] == 1 and log.counts[FLAGS] == 1 and log.counts[ROWS] == 2 and log.counts["segtopk_merge_kernel"] == 1
        K = min(B, seg)
        assert out["rows"].shape == (A_t, K, W) and out["beam"].shape == (A_t, K, S_t + 1) and out["logit"].shape == (A_t, K)
        assert out["n_candidates"] == len(rows) and out["n_invalid"] == int(bad.sum()) and out["n_twins"] == int((tw & ~bad).sum())
        assert out["n_excluded"] == 0
        z = {key: out[key].cpu().numpy() for key in ("rows", "logit", "proba", "rank", "parent", "added", "count", "beam")}
        for k in range(A_t):
            ok = np.flatnonzero(~(bad | tw)[k * seg:(k + 1) * seg])
            l = ref[k * seg + ok].astype(np.float64)
            count = int(z["count"][k])
            print(f"case {case} {mode} step {t} seed {active[k]}: {len(ok)} valid non-twin candidates, {count} kept")
            assert count == min(B, len(ok))
            theta = np.sort(l)[::-1][B - 1] if len(l) >= B else -np.inf
            m = TOL * np.abs(l).max()
            rank = z["rank"][k, :count]
            assert np.isin(rank, ok).all() and len(set(rank.tolist())) == count
            assert np.isin(ok[l > theta + 2 * m], rank).all(), (case, mode, t, k)
            assert (ref[k * seg + rank] >= theta - 2 * m).all(), (case, mode, t, k)
            logit = z["logit"][k, :count]
            e = logit_err(logit, ref[k * seg + rank])
            assert e <= TOL, (case, mode, t, k, e)
            assert (np.diff(logit) <= 0).all()
            assert np.array_equal(z["rows"][k, :count], rows[k * seg + rank]) and np.array_equal(z["beam"][k], z["rows"][k, :, :S_t + 1])
            assert np.array_equal(rank, z["parent"][k, :count] * n + z["added"][k, :count] - lo)
            for row, parent, add in zip(z["rows"][k, :count].tolist(), z["parent"][k, :count].tolist(), z["added"][k, :count].tolist()):
                assert sorted(CR.leading_ids(beam[k, parent]) + [add]) == [v for v in row if v]
            assert (z["rank"][k, count:] == -1).all() and not z["rows"][k, count:].any() and not z["logit"][k, count:].any()
            assert not z["parent"][k, count:].any() and not z["added"][k, count:].any() and not z["proba"][k, count:].any()
        kept = out["rank"] >= 0
        assert torch.equal(out["proba"][kept], torch.sigmoid(out["logit"][kept]))


# ---- the whole growth against the Python twin on the device's own logits ------------------------------------------------------------
@pytest.fixture(scope="module")
def d64():
    """The d = 64 table model of tests/test_hip_kway.py on hg38 at 1 Mb; the 48-bin chromosome is the region."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    cr = np.asarray(synth.chrom_range(num))
    c = num.index(48)
    clf, _ = hip_model(num, 64, "table", 12)
    P, fe, _ = oracle_state(num, 64, "table", 12)
    return dict(clf=clf.eval(), lo=int(cr[c][0]), hi=int(cr[c][1]), N=int(np.sum(num)), chr1=(int(cr[0][0]), int(cr[0][1])), oracle=(P, fe))


def device_score(clf, width):
    def score(rows):
        assert rows.shape[1] == width
        with torch.no_grad(), _lib.option("disable_small_batch"):
            return clf(torch.from_numpy(rows).cuda()).reshape(-1).cpu().numpy()
    return score


def check_growth(clf, oracle, seeds, lo, hi, max_size, beam, gap, width, long_rows):
    clf.eval()
    ref = GR.grow(seeds, lo, hi - lo, max_size, beam, gap, width, device_score(clf, width))
    first = None
    for chunk_rows in (None, 37, 4099):
        with _lib.launch_log() as log:
            out = SW.growth_sweep(clf, seeds, lo, hi, max_size, beam=beam, min_gap=gap, width=width, chunk_rows=chunk_rows)
        ran = {name for name, c in log.counts.items() if c > 0}
        if out["steps"]:
            assert (LONG <= ran and not (ran & SHORT_ONLY)) if long_rows else (ran & SHORT_ONLY and not (ran & LONG)), sorted(ran)
            assert log.counts[TWINS] == out["steps"] and not any(word in name for name in ran for word in ("bwd", "adamw")), sorted(ran)
        if first is None:
            first = out
        else:                                                            # the cut is not part of the result
            assert all(torch.equal(out[key], first[key]) for key in KEYS), (width, chunk_rows)
            assert all(out[key] == first[key] for key in INTS)
    z = {key: first[key].cpu().numpy() for key in KEYS}
    for key in ("rows", "logit", "parent", "added", "count", "size", "path"):
        assert z[key].shape == ref[key].shape and z[key].dtype == ref[key].dtype and np.array_equal(z[key], ref[key]), key      # bit for bit
    assert all(first[key] == ref[key] for key in INTS), [(first[key], ref[key]) for key in INTS]
    kept = np.arange(beam).reshape(1, 1, -1) < z["count"][:, :, None]
    assert np.array_equal(z["proba"][kept], torch.sigmoid(first["logit"]).cpu().numpy()[kept]) and not z["proba"][~kept].any()
    if kept.any():                                                       # every returned row against the fp32 oracle at that width
        P, fe = oracle
        with torch.no_grad():
            lg, _ = O.classifier_forward(P, fe, torch.from_numpy(z["rows"][kept]), random_chrom=0)
        e = logit_err(z["logit"][kept], lg.numpy().reshape(-1))
        print(f"width {width}: {int(kept.sum())} kept rows, logit_err against the oracle {e:.2e}")
        assert e <= TOL, e
    ids = [sorted(int(v) for v in s if int(v)) for s in seeds]
    for a, s in enumerate(ids):                                          # path replays to the last level's rows
        levels = int((z["size"][a] > 0).sum())
        assert levels == (max_size - len(s) if 1 <= len(s) < max_size else 0)
        if levels:
            c = int(z["count"][a, levels - 1])
            for j in range(c):
                assert sorted(s + [int(v) for v in z["path"][a, j, :levels]]) == [int(v) for v in z["rows"][a, levels - 1, j] if v]
            assert not z["path"][a, c:].any() and not z["path"][a, :, levels:].any()
        else:
            assert not z["path"][a].any() and not z["count"][a].any()
    return first


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_growth_is_the_twin_on_the_tiny_models(mode):
    clf = load_tiny(mode)
    oracle = golden_oracle(mode)
    rng = np.random.default_rng(31)
    pick = lambda s: sorted(int(v) for v in rng.choice(np.arange(1, 65), size=s, replace=False))
    # width 8, the short forward: ragged seeds, one at max_size, an empty one
    out = check_growth(clf, oracle, [pick(1), pick(3), pick(6), [], pick(4)], 17, 49, 6, 4, 1, 8, False)
    assert out["steps"] == 5 and out["n_twins"] > 0 and out["n_invalid"] > 0 and int(out["count"].sum()) == 4 * (5 + 3 + 2)
    # width 16, the long forward, min_gap 2; a region of 3 bins: count < beam, empty slots propagate
    check_growth(clf, oracle, [[2, 9], pick(1), [5, 8, 30, 33, 40, 44, 50, 52, 60, 62, 64]], 1, 65, 13, 3, 2, 16, True)
    small = check_growth(clf, oracle, [[40], [2, 3], [20, 22, 30]], 20, 23, 5, 8, 1, 16, True)
    assert small["count"][0].tolist() == [3, 3, 1, 0] and small["count"][1].tolist() == [3, 3, 1, 0] and small["count"][2].tolist() == [1, 0, 0, 0]
    assert small["rows"].shape == (3, 4, 8, 16) and small["steps"] == 4


def test_growth_is_the_twin_on_d64(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    rng = np.random.default_rng(41)
    pool = np.concatenate([np.arange(*d64["chr1"]), np.arange(lo, hi)])
    pick = lambda s: sorted(int(v) for v in rng.choice(pool, size=s, replace=False))
    out = check_growth(clf, d64["oracle"], [pick(29), pick(26), pick(32 - 1), [], pick(30)], lo, hi, 32, 8, 1, 32, True)
    assert out["steps"] == 6 and out["rows"].shape == (5, 6, 8, 32) and out["size"][1].tolist() == [27, 28, 29, 30, 31, 32]
    check_growth(clf, d64["oracle"], [pick(1), pick(2), pick(5), pick(3)], lo, hi, 5, 5, 3, 8, False)
    check_growth(clf, d64["oracle"], torch.tensor([[lo + 4, 0, 0], [lo + 1, lo + 9, d64["chr1"][0]]], device="cuda"), lo, lo + 3, 6, 8, 1, 16, True)


# ---- exclusion, errors, the other sweeps ------------------------------------------------------------------------------------------------
def test_exclude_with_a_wide_set(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    n, gap, W = hi - lo, 1, 32
    rng = np.random.default_rng(5)
    pool = np.arange(*d64["chr1"])
    beam = np.stack([random_beam(rng, 1, 4, 9, lo, n, np.concatenate([pool, np.arange(lo, hi)]))[0] for _ in range(3)])
    rows, bad, tw = GR.candidates(beam, lo, n, gap, W)
    free = ~(bad | tw)
    assert free.any() and tw.any() and bad.any()
    known = np.concatenate([np.flatnonzero(free)[::5], np.flatnonzero(bad)[::3], np.flatnonzero(tw & ~bad)[::2]])
    hset = HyperedgeSet(torch.from_numpy(rows[known]).cuda())
    assert hset.L == 32
    seg = 4 * n
    out = SW.grow_step(clf, beam, lo, hi, beam_out=64, min_gap=gap, width=W, exclude=hset, chunk_rows=50)
    # a twin's row is its elder's row: excluding it excludes the elder too, and only valid non-twin candidates count
    in_set = np.asarray([tuple(r) in {tuple(q) for q in rows[known]} for r in rows])
    assert out["n_excluded"] == int((in_set & free).sum()) >= len(np.flatnonzero(free)[::5])
    assert out["n_invalid"] == int(bad.sum()) and out["n_twins"] == int((tw & ~bad).sum()) and out["n_candidates"] == len(rows)
    left = free & ~in_set
    for a in range(3):
        want = np.flatnonzero(left[a * seg:(a + 1) * seg])
        got = out["rank"][a, :int(out["count"][a])].tolist()
        assert int(out["count"][a]) == min(64, len(want)) == len(set(got)) and set(got) <= set(want.tolist())
    everything = SW.grow_step(clf, beam, lo, hi, beam_out=64, min_gap=gap, width=W)
    assert everything["n_excluded"] == 0 and int(everything["count"].sum()) == sum(min(64, int(free[a * seg:(a + 1) * seg].sum())) for a in range(3))
    grown = SW.growth_sweep(clf, beam[:, 0], lo, hi, 11, beam=4, min_gap=gap, width=W, exclude=hset)
    plain = SW.growth_sweep(clf, beam[:, 0], lo, hi, 11, beam=4, min_gap=gap, width=W)
    assert plain["n_excluded"] == 0 and grown["n_candidates"] == plain["n_candidates"] == 3 * n + 3 * 4 * n
    reg = SW.growth_sweep(clf, beam[:, 0], lo, hi, 11, beam=4, min_gap=gap, width=W, task_mode="regress")
    kept = reg["added"] > 0
    assert torch.equal(reg["rows"], plain["rows"]) and torch.equal(reg["logit"], plain["logit"]) and bool(kept.any())
    assert torch.equal(reg["proba"][kept], torch.nn.functional.softplus(reg["logit"][kept])) and not reg["proba"][~kept].any()


def test_errors_and_empty_cases(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    seeds = [[d64["chr1"][0] + 3, lo + 5], [lo + 7]]
    beam = torch.tensor([[[lo + 1, lo + 5]], [[lo + 7, 0]]])
    clf._runtime()                                                       # (packing the model's parameters is not the sweep's doing)
    with _lib.launch_log() as log:
        for kw in (dict(max_size=1), dict(max_size=33), dict(max_size=6, beam=0), dict(max_size=6, beam=65), dict(max_size=6, width=5),
                   dict(max_size=6, width=33), dict(max_size=20, width=32, chunk_rows=1 << 27), dict(max_size=6, task_mode="other")):
            with pytest.raises(ValueError):
                SW.growth_sweep(clf, seeds, lo, hi, **kw)
        with pytest.raises(ValueError):
            SW.growth_sweep(clf, [list(range(1, 33))], lo, hi, 32)       # a seed of 32 ids
        for kw in (dict(width=2), dict(width=33), dict(beam_out=65), dict(width=32, chunk_rows=1 << 27)):
            with pytest.raises(ValueError):
                SW.grow_step(clf, beam, lo, hi, **kw)
        # no seeds, seeds without levels, an empty region
        for tab, reg, T in (([], (lo, hi), 0), ([[], [1, 2, 3, 4, 5, 6]], (lo, hi), 0), (seeds, (lo, lo), 5)):
            empty = SW.growth_sweep(clf, tab, *reg, 6, beam=4)
            assert empty["rows"].shape == (len(tab), T, 4, 6) and empty["path"].shape == (len(tab), 4, T) and empty["rows"].is_cuda
            assert all(empty[key] == 0 for key in INTS) and not empty["count"].any() and not empty["size"].any()
        none = SW.grow_step(clf, beam, lo, lo, beam_out=4)
        assert none["rows"].shape == (2, 0, 3) and none["beam"].shape == (2, 0, 3) and none["n_candidates"] == 0
        assert SW.grow_step(clf, torch.zeros(0, 2, 2, dtype=torch.long), lo, hi)["rows"].shape == (0, 2, 3)
    assert not log.counts
    with pytest.raises(IndexError):
        SW.growth_sweep(clf, [seeds[0], [3, d64["N"] + 5]], lo, hi, 4)   # a seed id beyond the model's table: once, at the end
    assert clf.check_ids                                                 # the per-call check is back on
    a, b = SW.growth_sweep(clf, seeds, lo, hi, 5, beam=5), SW.growth_sweep(clf, seeds, lo, hi, 5, beam=5)
    assert all(torch.equal(a[key], b[key]) for key in KEYS) and a["rows"].shape == (2, 4, 5, 5)


def test_the_other_sweeps_launch_what_they_launched(d64):
    clf, lo, hi = d64["clf"], d64["lo"], d64["hi"]
    with _lib.launch_log() as log:
        SW.anchored_sweep(clf, np.asarray([d64["chr1"][0], d64["chr1"][0] + 9]), lo, hi, 3, 3, top=10, chunk_rows=999)
    assert {"kway_anchor_rows_kernel", "segtopk_init_kernel", "segtopk_read_kernel"} | SEG_KERNELS <= set(log.counts)
    assert not {"kway_rows_kernel", ROWS, TWINS, FLAGS} & set(log.counts)
    assert log.counts["kway_anchor_rows_kernel"] == 3 + 1 and log.counts["segtopk_merge_kernel"] == 3      # 2 070 rows in chunks of 999
    with _lib.launch_log() as log:
        SW.completion_sweep(clf, [[d64["chr1"][0] + 2, lo + 3], [lo + 9]], lo, hi, top=5, chunk_rows=50)
    assert {ROWS, "segtopk_init_kernel", "segtopk_read_kernel"} | SEG_KERNELS <= set(log.counts)
    assert not {"kway_rows_kernel", "kway_anchor_rows_kernel", TWINS, FLAGS} & set(log.counts)
    assert log.counts[ROWS] == 2 + 2 and log.counts["segtopk_merge_kernel"] == 2 and log.counts["segtopk_init_kernel"] == 1      # 96 rows in chunks of 50


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_grow(tmp_path):
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
    away = np.asarray([v for v in range(1, 65) if not lo - 1 <= v <= hi])                 # the seed of 25 keeps clear of the region
    seeds = [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s, pool in ((1, np.arange(1, 65)), (9, np.arange(1, 65)), (25, away))]
    ipath = os.path.join(tmp_path, "seeds.txt")
    with open(ipath, "w") as f:
        for ids in seeds:
            items = []
            for v in rng.permutation(ids):                               # unsorted on the line, positions anywhere inside their bins
                c, s = node2bin[int(v)].split(":")
                items.append("%s:%d" % (c, int(s) + R.FIXTURE_RES // 3))
            f.write("\t".join(items) + "\n\n")                           # an empty line behind each: line numbers 1, 3, 5
    clf = load_tiny("table")

    def run(*extra):
        out = os.path.join(tmp_path, "grow.tsv")
        PR.main(["grow", "-i", ipath, "--chrom", "2", "--max-size", "27", "-o", out, "--config", cpath, *extra])
        with np.load(os.path.join(tmp_path, "grow.npz")) as f:           # read now: the next run writes the same file
            z = {key: f[key] for key in f.files}
        assert set(z) == {"seeds", *KEYS} and np.array_equal(z["seeds"], CR.padded(seeds))
        lines = [line.rstrip("\n").split("\t") for line in open(out)]
        assert len(lines) == int(z["count"].sum())
        at = 0
        for a in range(3):                                               # grouped by seed and size, best first
            for t in range(z["count"].shape[1]):
                for row, p in zip(z["rows"][a, t, :z["count"][a, t]], z["proba"][a, t, :z["count"][a, t]]):
                    size = int(z["size"][a, t])
                    assert int(lines[at][0]) == 2 * a + 1 and int(lines[at][1]) == size == len(seeds[a]) + t + 1
                    assert lines[at][2:2 + size] == [node2bin[int(v)] for v in row[:size]] and len(lines[at]) == size + 3
                    assert np.float32(float(lines[at][-1])) == p
                    at += 1
        return z

    def same(z, ref):
        return all(np.array_equal(z[key], ref[key].cpu().numpy()) for key in KEYS)

    z = run()
    assert z["rows"].shape == (3, 26, 8, 27) and z["size"][2].tolist() == [26, 27] + [0] * 24 and z["count"][2, 0] == 8
    assert same(z, SW.growth_sweep(clf, seeds, lo, hi, 27, beam=8, min_gap=1))              # min_gap = min_distance + 1
    w = run("--start-bin", "2", "--end-bin", "14", "--width", "32", "--chunk-rows", "50", "--beam", "3", "--min-gap", "2")
    assert w["rows"].shape == (3, 26, 3, 32)
    assert same(w, SW.growth_sweep(clf, seeds, lo + 2, lo + 14, 27, beam=3, min_gap=2, width=32))
    # --exclude-known drops the rows of all_<k>_counter.npy for the sizes present (2 .. 27 here; only 2 and 26 have a file)
    np.save(os.path.join(temp, "all_2_counter.npy"), z["rows"][0, 0, [0, 3], :2])
    np.save(os.path.join(temp, "all_26_counter.npy"), z["rows"][2, 0, [1], :26])
    e = run("--exclude-known")
    more = SW.growth_sweep(clf, seeds, lo, hi, 27, beam=10, min_gap=1)["rows"].cpu().numpy()
    assert np.array_equal(e["rows"][0, 0], more[0, 0][[1, 2, 4, 5, 6, 7, 8, 9]]) and np.array_equal(e["rows"][2, 0], more[2, 0][[0, 2, 3, 4, 5, 6, 7, 8]])
    assert np.array_equal(e["rows"][1, 0], more[1, 0, :8])
