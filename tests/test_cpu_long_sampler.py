"""The membership set and the negative sampler for rows of up to 32 columns, without a GPU: the ABI surface, the refusals of the three
`_long` entry points (before any device call), and the plain-Python twin tests/sampler_long_ref.py -- bit for bit against oracle/sampler.py
at L <= 8, the invariants of generate_negative at L in {9, 17, 32}, and its distribution against the reference's own statistics."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from matcha_amd import _lib, synth
from tests import sampler_long_ref as SL
from tests.helpers import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = ("matcha_hashset_build_long", "matcha_hashset_contains_long", "matcha_neg_sample_long")
EINVAL = -22


def _header():
    return open(os.path.join(ROOT, "include", "matcha_hip.h")).read()


def test_abi_holds_the_three_long_entry_points_at_version_7():
    hdr = _header()
    assert "#define MATCHA_ABI_VERSION 7" in hdr and "#define MATCHA_MAX_L 8 " in hdr and "#define MATCHA_MAX_LONG_L 32" in hdr
    assert int(re.search(r"#define MATCHA_EINVAL \(?(-?\d+)\)?", hdr).group(1)) == EINVAL
    lib = _lib.load()
    assert lib.matcha_abi_version() == _lib.ABI_VERSION == 7
    short = {"matcha_hashset_build_long": "matcha_hashset_build", "matcha_hashset_contains_long": "matcha_hashset_contains",
             "matcha_neg_sample_long": "matcha_neg_sample"}
    for name in LONG:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name] == _lib.SIGNATURES[short[name]]      # the parameter list of the short twin
        assert getattr(lib, name) is not None
        # ... in the header too: the same parameter types in the same order
        def params(n):
            body = re.search(r"\bint %s\((.*?)\);" % n, hdr, re.S).group(1)
            return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", q.strip())).strip() for q in body.split(",")]
        assert params(name) == params(short[name]), name


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_long_entry_points_refuse_bad_arguments_before_any_device_call():
    """Host buffers stand in for device memory: every call below must return MATCHA_EINVAL with a message and touch nothing."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, dtype=np.int64)               # 512 KiB, 8-byte aligned
    x = np.zeros(4096, dtype=np.int64)
    out = np.zeros(64, dtype=np.int32)
    n2c = np.zeros(64, dtype=np.int32)
    cr = np.zeros(64, dtype=np.int32)
    seed = np.zeros(1, dtype=np.uint64)
    need = lib.matcha_hashset_bytes(3)
    assert need <= buf.nbytes

    def refused(rc, word):
        msg = lib.matcha_last_error()
        assert rc == EINVAL and word in msg, (rc, msg)

    # build: L = 0, L = 33, null pointers, a too-small set buffer
    refused(lib.matcha_hashset_build_long(_p(buf), need, _p(x), 3, 0, None), b"matcha_hashset_build_long: L=0")
    refused(lib.matcha_hashset_build_long(_p(buf), need, _p(x), 3, 33, None), b"matcha_hashset_build_long: L=33")
    refused(lib.matcha_hashset_build_long(None, need, _p(x), 3, 9, None), b"matcha_hashset_build_long: null pointer")
    refused(lib.matcha_hashset_build_long(_p(buf), need, None, 3, 9, None), b"matcha_hashset_build_long: null pointer")
    refused(lib.matcha_hashset_build_long(_p(buf), 16, _p(x), 100, 9, None), b"matcha_hashset_build_long: set buffer too small")
    refused(lib.matcha_hashset_build_long(_p(buf), need, _p(x), -1, 9, None), b"n_edges")
    # the short entry keeps its bound
    refused(lib.matcha_hashset_build(_p(buf), need, _p(x), 3, 9, None), b"matcha_hashset_build: L=9")
    refused(lib.matcha_hashset_contains(_p(buf), _p(x), 9, _p(x), 4, 3, _p(out), None), b"matcha_hashset_contains: bad width")
    # contains: both widths in 1 .. 32, null pointers
    for L_set, L in ((33, 9), (9, 33), (0, 9), (9, 0)):
        refused(lib.matcha_hashset_contains_long(_p(buf), _p(x), L_set, _p(x), 4, L, _p(out), None), b"matcha_hashset_contains_long: bad width")
    refused(lib.matcha_hashset_contains_long(None, _p(x), 9, _p(x), 4, 9, _p(out), None), b"matcha_hashset_contains_long: null pointer")
    refused(lib.matcha_hashset_contains_long(_p(buf), _p(x), 9, None, 4, 9, _p(out), None), b"matcha_hashset_contains_long: null pointer")
    refused(lib.matcha_hashset_contains_long(_p(buf), _p(x), 9, _p(x), 4, 9, None, None), b"matcha_hashset_contains_long: null pointer")

    # sample: L = 0 / 33, L_set = 33, null pointers, a misaligned chrom_range, neg_num = 0, a non-empty set without buffers
    def sample(set_=_p(buf), edges=_p(x), n_set=3, L_set=9, pos=_p(x), P=8, L=9, neg_num=3, n2c_=_p(n2c), cr_=_p(cr), seed_=_p(seed), neg=_p(x)):
        return lib.matcha_neg_sample_long(set_, edges, n_set, L_set, pos, P, L, neg_num, 0, n2c_, 10, cr_, 1, seed_, neg, _p(out), None)

    refused(sample(L=0), b"matcha_neg_sample_long: L=0")
    refused(sample(L=33), b"matcha_neg_sample_long: L=33")
    refused(sample(L_set=33), b"matcha_neg_sample_long: L_set=33")
    refused(sample(L_set=0), b"matcha_neg_sample_long: L_set=0")
    refused(sample(neg_num=0), b"neg_num=0")
    for kw in ("pos", "neg", "n2c_", "cr_", "seed_"):
        refused(sample(**{kw: None}), b"matcha_neg_sample_long: null pointer")
    refused(sample(cr_=C.c_void_p(cr.ctypes.data + 4)), b"chrom_range must be 8-byte aligned")
    refused(sample(set_=None), b"non-empty set without buffers")
    refused(sample(edges=None), b"non-empty set without buffers")
    refused(sample(P=1 << 30, neg_num=3), b"negatives")
    assert not buf.any() and not x.any() and not out.any()               # nothing was written


def _case(layout, ks, m, L=None):
    num = synth.LAYOUTS[layout]
    N = int(np.sum(num))
    rng = np.random.default_rng(3)
    L = L or max(ks)
    pool = np.concatenate([np.pad(synth.make_edges_fast(rng, N, k, m), ((0, 0), (0, L - k))) for k in ks])
    known = {tuple(int(v) for v in r if v) for r in pool}
    return num, N, L, pool, known


@pytest.mark.parametrize("layout,ks,min_dis", [("tiny", [2, 3], 0), ("c1", [2, 3, 4, 5], 0), ("c1", [3], 2), ("c1", [2, 5, 8], 1)])
def test_long_twin_equals_the_oracle_sampler_at_up_to_8_columns(layout, ks, min_dis):
    """The cases of tests/test_cpu_twins.py (L = 3, 5, 3, 8): with stride 8 the new twin IS oracle/sampler.py, bit for bit -- status too.
    The last case (min_dis 1 at k up to 8) holds positives whose unchanged nodes are adjacent: each such negative burns all 65 536 trials
    in both Python restatements, so that case takes 50 positives, not 200."""
    from oracle import sampler as OS
    num, N, L, pool, known = _case(layout, ks, 150 if layout == "tiny" else 400)
    assert L <= 8 and SL.stride_of(L) == 8 and SL.stride_of(9) == 32
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    pos = pool[np.random.default_rng(2).permutation(len(pool))[:50 if min_dis == 1 else 200]]
    fresh = np.pad(synth.make_edges_fast(np.random.default_rng(9), N, ks[0], 20), ((0, 0), (0, L - ks[0])))
    pos = np.concatenate([pos, fresh])
    neg, status = SL.sample_negatives_long(pos, known, n2c, cr, 3, min_dis, 42, return_status=True)
    ref = OS.sample_negatives(pos, known, n2c, cr, 3, min_dis, seed=42)
    assert np.array_equal(neg, ref)
    exhausted = sum(1 for n in range(len(neg)) if np.array_equal(neg[n], pos[n // 3]) and tuple(int(v) for v in pos[n // 3] if v) in known)
    assert status[0] == 0 and status[1] == exhausted
    assert np.array_equal(SL.sample_negatives_long(pos, set(), n2c, cr, 3, min_dis, 42), np.repeat(pos, 3, axis=0))


@pytest.mark.parametrize("L", [2, 5, 8])
def test_long_twin_equals_the_oracle_sampler_at_each_short_width(L):
    from oracle import sampler as OS
    num, N, L, pool, known = _case("c1", [2, L] if L > 2 else [2], 300, L)
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    pos = pool[np.random.default_rng(4).permutation(len(pool))[:150]]
    assert np.array_equal(SL.sample_negatives_long(pos, known, n2c, cr, 3, 0, 7), OS.sample_negatives(pos, known, n2c, cr, 3, 0, seed=7))


@pytest.mark.parametrize("L", [9, 17, 32])
@pytest.mark.parametrize("min_dis", [0, 2])
def test_long_twin_keeps_the_invariants_of_generate_negative(L, min_dis):
    """SURVEY.md 8 c3 on rows of 9, 17 and 32 columns (k = 32 takes the full 32-bit mask): same k as the positive, ascending and
    duplicate-free, gaps > min_dis, not known, the same chromosome multiset, at least one node changed; a non-member is copied."""
    num = synth.LAYOUTS["hg38_1mb"]
    N = int(np.sum(num))
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    rng = np.random.default_rng(50 + L)
    ks = sorted({2, 8, 9, L - 1, L})
    rows = []
    for k in ks:
        v = synth.make_edges_fast(rng, N, k, 120)
        v = v[(np.diff(v, axis=1) > min_dis).all(axis=1)][:40]
        rows.append(np.pad(v, ((0, 0), (0, L - k))))
    pool = np.concatenate(rows)
    known = {tuple(int(v) for v in r if v) for r in pool[::2]} | {tuple(int(v) for v in pool[-1] if v)}      # every other row is known
    neg, status = SL.sample_negatives_long(pool, known, n2c, cr, 3, min_dis, 5, return_status=True)
    assert status.tolist() == [0, 0, 0, 0]
    checked = SL.check_invariants(pool, neg, known, n2c, 3, min_dis)
    assert checked == 3 * sum(1 for r in pool if tuple(int(v) for v in r if v) in known) and checked >= 3 * len(pool) // 2
    # a function of (seed, n, the positive, L, the set's contents): the same rows again, another seed differs
    assert np.array_equal(neg, SL.sample_negatives_long(pool, known, n2c, cr, 3, min_dis, 5))
    assert not np.array_equal(neg, SL.sample_negatives_long(pool, known, n2c, cr, 3, min_dis, 6))


def test_stride_32_does_not_reuse_a_draw_between_trials():
    """At stride 8, position 8 of trial t and position 0 of trial t + 1 share a counter; at stride 32 no two (trial, position) pairs do, and
    the last replacement counter stays below the mask counters."""
    assert 8 * 0 + 8 == 8 * 1 + 0
    ctr = {32 * t + p for t in (0, 1, 2, 65535) for p in range(32)}
    assert len(ctr) == 4 * 32 and max(ctr) == 32 * 65535 + 31 < 0xFFFF0000


def long_statistics_against_reference(batch, neg, min_dis, ks=(9, 12, 16, 25)):
    """{k: ((chi2 of the differing-node histogram, bins), (chi2 of the replaced-position histogram, bins))} against
    tests/golden/sampler_stats_long.npz, each asserted below scipy.stats.chi2.isf(1e-6, bins - 1)."""
    from scipy.stats import chi2
    g = gold("sampler_stats_long.npz")
    diff, posh = SL.statistics(batch, neg, 3, ks)
    out = {}
    for k in ks:
        rd, rp = g[f"long_d{min_dis}_diff_k{k}"], g[f"long_d{min_dis}_pos_k{k}"]
        assert diff[k].sum() == rd.sum() == 3000 and diff[k][0] == 0 and rd[0] == 0
        (c_d, b_d), (c_p, b_p) = SL.chi2_two_sample(diff[k], rd), SL.chi2_two_sample(posh[k], rp)
        print(f"long sampler statistics min_dis {min_dis} k {k}: diff chi2 {c_d:.2f} ({b_d} bins, bound {chi2.isf(1e-6, b_d - 1):.2f}), "
              f"positions chi2 {c_p:.2f} ({b_p} bins, bound {chi2.isf(1e-6, b_p - 1):.2f})")
        assert c_d < chi2.isf(1e-6, b_d - 1) and c_p < chi2.isf(1e-6, b_p - 1), (k, c_d, b_d, c_p, b_p)
        out[k] = ((c_d, b_d), (c_p, b_p))
    return out


@pytest.mark.parametrize("min_dis", [0, 2])
def test_long_twin_distribution_vs_reference(min_dis):
    """Fixture sampler_stats_long.npz: the reference's own generate_negative (main.py:361-459) on ONE mixed batch of k in {9, 12, 16, 25}
    padded to 25 (hg38 1 Mb, neg_num 3, min_dis 0 / 2, 1 000 positives and 3 000 negatives per k).  The twin draws from another random
    stream, so the comparison is distributional: per k the histogram of how many nodes a negative differs in and of which position was
    replaced -- two-sample chi-square sum (a - b)^2 / (a + b), bins with fewer than 10 counts together pooled, bound
    chi2.isf(1e-6, bins - 1) -- with every invariant asserted on the way.

    Measured (seed 11; both streams are deterministic) -- chi2 [bins used; bound] of the differing-node / replaced-position histograms:
      min_dis 0: k 9  15.82 [9; 42.70] / 3.16 [9; 42.70]     k 12 14.38 [12; 48.87] / 4.42 [12; 48.87]
                 k 16 11.97 [13; 50.83] / 11.63 [16; 56.49]  k 25 15.55 [16; 56.49] / 13.97 [25; 72.23]
      min_dis 2: k 9  7.46 [9; 42.70] / 4.96 [9; 42.70]      k 12 4.28 [11; 46.86] / 2.99 [12; 48.87]
                 k 16 10.01 [14; 52.75] / 6.76 [16; 56.49]   k 25 16.57 [15; 54.64] / 7.92 [25; 72.23]"""
    num = synth.LAYOUTS["hg38_1mb"]
    n2c, cr = synth.node2chrom(num), synth.chrom_range(num)
    batch, known, _ = SL.long_sampler_case(min_dis)
    neg = SL.sample_negatives_long(batch, known, n2c, cr, 3, min_dis, 11)
    assert SL.check_invariants(batch, neg, known, n2c, 3, min_dis) == len(neg)
    long_statistics_against_reference(batch, neg, min_dis)
