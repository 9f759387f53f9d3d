"""Cluster growth without a GPU (matcha_amd/sweep.py, csrc/grow.hip's host side): the two entry points and their refusals
before any device call, the twin rule's "exactly one non-twin per distinct row" on random beams (tests/grow_ref.py), the g17 fixture's
consistency, the fp32 oracle on its rows, and the wrappers' and the CLI's checks.  (The host side alone under ASan + UBSan: tests/test_cpu_host_checks.py.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR
from matcha_amd import sweep as SW
from oracle import hypersagnn as O
from tests import complete_ref as CR
from tests import grow_ref as GR
from tests.helpers import gold, logit_err
from tests.test_cpu_long_rows import golden_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_header_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "matcha_hip.h")).read()
    lib = _lib.load()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and lib.matcha_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("matcha_grow_twins", "matcha_grow_twin_flags"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)


def test_argument_errors_refused_without_a_device():
    lib = _lib.load()
    host = (C.c_int64 * 64)()                                            # never dereferenced: every call below is refused first
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.matcha_last_error().decode()
    twins = lambda *a: lib.matcha_grow_twins(*a, None)
    flags = lambda *a: lib.matcha_grow_twin_flags(*a, None)
    with _lib.launch_log() as log:
        # beam, A, B, S, twin
        assert twins(p, 4, 0, 9, p) == -22 and "B=" in err()
        assert twins(p, 4, 65, 9, p) == -22 and "B=" in err()
        assert twins(p, 4, 8, 0, p) == -22 and "S=" in err()
        assert twins(p, 4, 8, 32, p) == -22 and "S=" in err()
        assert twins(p, -1, 8, 9, p) == -22 and "A=" in err()
        assert twins(None, 4, 8, 9, p) == -22 and "null beam" in err()
        assert twins(p, 4, 8, 9, None) == -22 and "null output" in err()
        assert twins(None, 0, 8, 9, None) == 0                                                                    # A = 0: a no-op
        # twin, A, B, lo, n, rank0, count, flag
        assert flags(p, 4, 0, 1, 16, 0, 4, p) == -22 and "B=" in err()
        assert flags(p, 4, 65, 1, 16, 0, 4, p) == -22 and "B=" in err()
        assert flags(p, 4, 8, 1, 0, 0, 0, p) == -22 and "n=" in err()                                             # n < 1
        assert flags(p, -1, 8, 1, 16, 0, 0, p) == -22 and "A=" in err()
        assert flags(p, 4, 8, -1, 16, 0, 4, p) == -22 and "lo" in err()
        assert flags(p, 4, 8, 1, 16, 510, 4, p) == -22 and "outside" in err()                                     # 4 * 8 * 16 = 512 ranks
        assert flags(p, 4, 8, 1, 16, -1, 1, p) == -22 and "outside" in err()
        assert flags(p, 4, 8, 1, 16, 513, 0, p) == -22 and "outside" in err()
        assert flags(p, 4, 8, 1, 16, 0, -1, p) == -22 and "count" in err()
        assert flags(p, 1 << 40, 64, 1, 1 << 17, 0, 1, p) == -22 and "63 bits" in err()                           # A B n = 2^63
        assert flags(None, 4, 8, 1, 16, 0, 4, p) == -22 and "null twin" in err()
        assert flags(p, 4, 8, 1, 16, 0, 4, None) == -22 and "null flag" in err()
        assert flags(p, 4, 8, 1, 16, 0, 0, None) == 0 and flags(p, 4, 8, 1, 16, 512, 0, None) == 0                # count = 0
        assert flags(None, 0, 8, 1, 16, 0, 0, None) == 0                                                          # A = 0
        assert flags(p, (1 << 40) - 1, 64, 1, 1 << 17, 0, 0, None) == 0                                           # just below 2^63
    assert not log.counts


def test_wrappers_refuse_before_any_launch():
    beam = torch.zeros(2, 3, 4, dtype=torch.long)
    with _lib.launch_log() as log:
        for bad in (torch.zeros(2, 65, 4, dtype=torch.long), torch.zeros(2, 3, 32, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long),
                    torch.zeros(2, 3, 4, dtype=torch.int32)):
            with pytest.raises(ValueError):
                SW.grow_twins(bad)
        with pytest.raises(_lib.MatchaHipError):
            SW.grow_twins(beam)                                          # every argument is fine: no CPU fallback
        twin, flag = torch.zeros(6, 3, dtype=torch.long), torch.zeros(6 * 16, dtype=torch.int32)
        for kw in (dict(rank0=95, count=2), dict(rank0=-1, count=1), dict(count=-1)):
            with pytest.raises(IndexError):
                SW.grow_twin_flags(twin, 1, 16, flag, **kw)
        for args in ((twin, 1, 0, flag), (torch.zeros(7, 3, dtype=torch.long), 1, 16, flag), (twin, 1, 16, flag[:95]),
                     (twin, 1, 16, flag.to(torch.int64))):
            with pytest.raises(ValueError):
                SW.grow_twin_flags(*args)
        with pytest.raises(_lib.MatchaHipError):
            SW.grow_twin_flags(twin, 1, 16, flag)
        # growth_sweep and grow_step check their arguments before they touch the model
        for kw in (dict(max_size=1), dict(max_size=33), dict(max_size=6, beam=0), dict(max_size=6, beam=65), dict(max_size=6, width=5),
                   dict(max_size=6, width=33), dict(max_size=6, min_gap=0), dict(max_size=6, chunk_rows=0), dict(max_size=6, task_mode="other")):
            with pytest.raises(ValueError):
                SW.growth_sweep(None, [[3, 4]], 1, 17, **kw)
        for kw in (dict(beam_out=0), dict(beam_out=65), dict(width=4), dict(width=33), dict(min_gap=0), dict(chunk_rows=0), dict(task_mode="other")):
            with pytest.raises(ValueError):
                SW.grow_step(None, beam, 1, 17, **kw)
        with pytest.raises(ValueError):
            SW.grow_step(None, torch.zeros(2, 65, 4, dtype=torch.long), 1, 17)
    assert not log.counts


def random_beam(rng, A, B, S, lo, n, pool):
    """Beams as a growth makes them: every slot of a seed is the seed's own ids and as many bins of the region as the others hold, so
    slots of one seed differ in region bins only; repeated slots are likely (few bins to choose from)."""
    beam = np.zeros((A, B, S), dtype=np.int64)
    for a in range(A):
        extra = int(rng.integers(0, S))
        own = rng.choice(np.setdiff1d(pool, np.arange(lo, lo + n)), size=S - extra, replace=False)
        for j in range(B):
            beam[a, j] = np.sort(np.concatenate([own, rng.choice(np.arange(lo, lo + n), size=extra, replace=False)]))
    return beam


def test_exactly_one_candidate_per_distinct_row_is_not_a_twin():
    rng = np.random.default_rng(17)
    checked = twins = 0
    for trial in range(60):
        A, B, S = int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(1, 7))
        lo, n = 5, int(rng.integers(S + 1, 9))
        beam = random_beam(rng, A, B, S, lo, n, np.arange(1, 40))
        rows, bad, tw = GR.candidates(beam, lo, n, 1, S + 1)
        table = GR.twin_table(beam)
        for a in range(A):
            seen = {}
            for q in range(B * n):
                g = a * B * n + q
                j, new_id = q // n, lo + q % n
                # the table says what the set rule says
                row = table[a * B + j]
                assert bool(((row[:j] == new_id) | (row[:j] == -1)).any()) == bool(tw[g]) and not row[j:].any()
                if not bad[g]:
                    seen.setdefault(tuple(rows[g]), []).append(g)
            for row, ranks in seen.items():
                assert not tw[ranks[0]] and tw[ranks[1:]].all(), (beam[a], row, ranks)      # the lowest slot's candidate, and it alone
                checked += 1
                twins += len(ranks) - 1
    assert checked > 1000 and twins > 300
    # slots that are not strictly ascending, empty slots and slots of another size have no twins and are nobody's twin
    odd = np.asarray([[[3, 4, 9], [3, 4, 4], [9, 4, 3], [0, 0, 0], [3, 4, 0], [3, 9, 0], [3, 4, 9], [4, 9, 11]]])
    assert np.array_equal(GR.twin_table(odd)[:, :7], [[0] * 7, [0] * 7, [0] * 7, [0] * 7, [0] * 7, [0, 0, 0, 0, 4, 0, 0], [-1, 0, 0, 0, 0, 0, 0],
                                                      [3, 0, 0, 0, 0, 0, 3]])


def g17_step_arrays(g, i, mode):
    """[(t, active, beam int64 [A_t, B_t, S_t], logits float32 [A_t B_t n])] of one case and model."""
    return [(t, active, g[f"beam_{mode}_c{i}_t{t}"].astype(np.int64), g[f"logit_{mode}_c{i}_t{t}"]) for t, active, _, _ in GR.g17_steps(i)]


def test_fixture_is_self_consistent():
    g = gold("g17_grow_tiny.npz")
    assert [int(v) for v in g["num"]] == [16, 16, 16, 16] and int(g["seed_base"]) == GR.G17_SEED
    for i, ((lo, hi), B, gap, sizes, max_size, W) in enumerate(GR.G17_CASES):
        n = hi - lo
        seeds = GR.g17_seeds(i)
        assert [len(s) for s in seeds] == list(sizes) and np.array_equal(g[f"seeds_c{i}"].astype(np.int64), CR.padded(seeds))
        for mode in ("table", "adj"):
            steps = g17_step_arrays(g, i, mode)
            assert len(steps) == max_size - min(sizes)
            near = 0
            for (t, active, beam, lg), (_, _, B_t, S_t) in zip(steps, GR.g17_steps(i)):
                assert beam.shape == (len(active), B_t, S_t) and lg.dtype == np.float32 and lg.shape == (len(active) * B_t * n,)
                if t == 0:
                    assert np.array_equal(beam[:, 0], CR.padded([seeds[a] for a in active], S_t))
                rows, bad, tw = GR.candidates(beam, lo, n, gap, W)
                empty = np.repeat(~beam.reshape(-1, S_t).any(axis=1), n)
                assert np.array_equal(np.isnan(lg), empty) and not empty.any()            # every slot of these beams is filled
                res = GR.step(beam, lo, n, gap, W, B, lambda r: lg)
                assert (res["count"] == min(B, B_t * n)).all()
                if t + 1 < len(steps):                                   # beam t + 1 is the twin's selection on the stored logits
                    nxt_active, nxt = steps[t + 1][1], steps[t + 1][2]
                    keep = [k for k, a in enumerate(active) if a in nxt_active]
                    assert np.array_equal(nxt, res["beam"][keep][:, :, :nxt.shape[2]]) and not res["beam"][keep][:, :, nxt.shape[2]:].any()
                seg = B_t * n
                for k in range(len(active)):
                    ok = ~(bad | tw)[k * seg:(k + 1) * seg]
                    v = np.sort(lg[k * seg:(k + 1) * seg][ok].astype(np.float64))[::-1]
                    if len(v) > B:
                        near += int((np.abs(v - v[B - 1]) <= GR.G17_TOL * np.abs(v).max()).sum()) - 1
            assert near <= GR.G17_NEAR, (i, mode, near)


@pytest.mark.parametrize("mode", ["table", "adj"])
def test_oracle_reproduces_the_reference_on_the_fixture(mode):
    g = gold("g17_grow_tiny.npz")
    P, fe = golden_oracle(mode)
    with torch.no_grad():
        for i, ((lo, hi), B, gap, sizes, max_size, W) in enumerate(GR.G17_CASES):
            worst = 0.0
            for t, active, beam, ref in g17_step_arrays(g, i, mode):
                rows, _, _ = GR.candidates(beam, lo, hi - lo, gap, W)
                lg, _ = O.classifier_forward(P, fe, torch.from_numpy(rows), random_chrom=0)
                worst = max(worst, logit_err(lg.numpy().reshape(-1), ref))
            print(f"{mode} case {i}: logit_err {worst:.2e}")
            assert worst <= 1e-5, (mode, i, worst)


def test_twin_growth_on_a_made_up_score():
    """The whole growth of tests/grow_ref.py on a score that ties often (sum of ids mod 7): ragged seeds, a seed at max_size, an empty
    seed, a region of 3 bins where count < beam and empty slots propagate; path replays to the last level's rows."""
    score = lambda rows: (rows.sum(axis=1) % 7).astype(np.float32)
    seeds = [[9], [2, 30, 31], [], [1, 2, 3, 4, 5], [40, 41]]
    for (lo, n), beam in (((10, 3), 8), ((10, 12), 4)):
        out = GR.grow(seeds, lo, n, 5, beam, 1, 8, score)
        T = 4
        assert out["rows"].shape == (5, T, beam, 8) and out["steps"] == T
        assert np.array_equal(out["size"], [[2, 3, 4, 5], [4, 5, 0, 0], [0] * 4, [0] * 4, [3, 4, 5, 0]])
        assert not out["count"][[2, 3]].any() and (out["count"] <= beam).all()
        if n == 3:
            assert out["count"][0].tolist() == [3, 3, 1, 0]             # {9} + 1, 2, 3 bins of 3; nothing left to add at size 5
        for a, s in enumerate(seeds):
            levels = int((out["size"][a] > 0).sum())
            for t in range(levels):
                c = out["count"][a, t]
                kept = [tuple(v for v in r if v) for r in out["rows"][a, t, :c]]
                assert len(set(kept)) == c and all(len(r) == len(s) + t + 1 and set(s) <= set(r) for r in kept)      # no hub twice
                assert not out["rows"][a, t, c:].any() and not out["added"][a, t, c:].any()
            if levels:
                c = out["count"][a, levels - 1]
                for j in range(c):
                    assert sorted(s + [int(v) for v in out["path"][a, j, :levels]]) == [int(v) for v in out["rows"][a, levels - 1, j] if v]
                assert not out["path"][a, c:].any() and not out["path"][a, :, levels:].any()


def _write_lines(path, lines):
    with open(path, "w") as f:
        for loci in lines:
            f.write("\t".join("chr1:%d" % (b * 100 + 7) for b in loci) + "\n")


def test_cli_line_check(tmp_path):
    """``predict grow`` reads its seeds with ``complete``'s parser: 1 to 31 distinct bins per line, the line number in the error."""
    bin2node = {"chr1:%d" % (b * 100): b + 1 for b in range(64)}
    path = os.path.join(tmp_path, "seeds.txt")
    _write_lines(path, [[5], list(range(31)), [9, 3, 3, 20]])
    seeds, lines = PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
    assert seeds == [[6], list(range(1, 32)), [4, 10, 21]] and lines == [1, 2, 3]
    _write_lines(path, [[5], list(range(32))])
    with pytest.raises(ValueError, match=r"line 2 has 32 distinct bins"):
        PR.parse_cluster_file(path, bin2node, ["chr1"], 100)
    ap_error = pytest.raises(SystemExit)
    with ap_error:
        PR.main(["grow", "-i", path, "--chrom", "0"])                    # --max-size is required
