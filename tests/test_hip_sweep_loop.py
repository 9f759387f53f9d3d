"""The sweeps' shared loop on the MI355X (matcha_amd/sweep.py's "the loop"): every driver that has no launch-count test of
its own is run on a region of 12 bins cut into three chunks with a short last one.  The result must equal the one-chunk result bit for
bit, and the library's launches -- the rows kernel, the sink's kernels, the forward's -- must be the LAUNCHES literals, which were
recorded from the code as it stood before the drivers shared one loop: the counts are deterministic, so they hold without a margin."""
import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd import expected as EX
from matcha_amd import sweep as SW
from matcha_amd.sampler import HyperedgeSet

pytestmark = pytest.mark.gpu

K3, GAP = 3, 1                              # triples of 12 bins: C(12, 3) = 220 candidates, 100 + 100 + 20
MIN_COUNT = 5


def make_d64():
    """The d = 64 table model of tests/test_hip_complete.py on hg38 at 1 Mb; the sweeps run on the first 12 (or 24) bins of the 48-bin
    chromosome."""
    from tests.test_hip_model import hip_model
    num = synth.LAYOUTS["hg38_1mb"]
    cr = np.asarray(synth.chrom_range(num))
    clf, _ = hip_model(num, 64, "table", 12)
    lo = int(cr[num.index(48)][0])
    known = SW.kway_rows(lo, 12, K3, GAP)[::7].contiguous()              # every seventh triple is a known hyperedge
    return dict(clf=clf.eval(), lo=lo, chr1=int(cr[0][0]), hset=HyperedgeSet(known), n_known=int(known.shape[0]))


@pytest.fixture(scope="module")
def d64():
    return make_d64()


def parts(d):
    return [(d["lo"], d["lo"] + 6, 1), (d["lo"] + 6, d["lo"] + 12, 2)]   # 6 * C(6, 2) = 90 candidates, 40 + 40 + 10


def clusters(d):
    """15 clusters of 4 loci and 9 of 5, across chromosome 1 and the region: 15 * C(4, 2) = 9 * C(5, 2) = 90 candidates per size."""
    rng = np.random.default_rng(3)
    pool = np.concatenate([np.arange(d["chr1"], d["chr1"] + 40), np.arange(d["lo"], d["lo"] + 12)])
    return [sorted(int(v) for v in rng.choice(pool, size=s, replace=False)) for s in [4] * 15 + [5] * 9]


def beam(d):
    """A = 2 seeds, B = 2 slots, S = 2 ids per slot; the slots of a seed share an id, so they have twins: 2 * 2 * 12 = 48 candidates,
    20 + 20 + 8."""
    lo = d["lo"]
    return torch.tensor([[[lo + 1, lo + 4], [lo + 1, lo + 7]], [[d["chr1"] + 3, lo + 5], [lo + 5, lo + 9]]], dtype=torch.long)


def expected_dict(ex):
    out = {key: torch.from_numpy(ex.raw[key]) for key in ("count", "sum", "sumsq")}
    out.update(mean=torch.from_numpy(ex.mean), var=torch.from_numpy(ex.var), n_rows=ex.n_rows, n_rejected=ex.n_rejected)
    return out


def enriched(d, chunk_rows, **kw):
    out = EX.kway_enriched_sweep(d["clf"], d["lo"], d["lo"] + 12, K3, GAP, top=30, min_count=MIN_COUNT, exclude=d["hset"], chunk_rows=chunk_rows, **kw)
    out.update(expected_dict(out.pop("expected_table")))
    return out


# name -> (the call at one chunk_rows, the chunk_rows that cuts it into three)
CASES = {
    "kway_sweep": (lambda d, c: SW.kway_sweep(d["clf"], d["lo"], d["lo"] + 12, K3, GAP, top=30, chunk_rows=c), 100),
    "kway_sweep_exclude": (lambda d, c: SW.kway_sweep(d["clf"], d["lo"], d["lo"] + 12, K3, GAP, top=30, chunk_rows=c, exclude=d["hset"]), 100),
    "kway_map": (lambda d, c: SW.kway_map(d["clf"], d["lo"], d["lo"] + 12, K3, GAP, chunk_rows=c, exclude=d["hset"]), 100),
    "region_sweep": (lambda d, c: SW.region_sweep(d["clf"], parts(d), GAP, top=30, chunk_rows=c, exclude=d["hset"]), 40),
    "region_sweep_per_leading": (lambda d, c: SW.region_sweep(d["clf"], parts(d), GAP, top=4, chunk_rows=c, exclude=d["hset"], per_leading=True), 40),
    "region_map": (lambda d, c: SW.region_map(d["clf"], parts(d), GAP, 0, 1, chunk_rows=c, exclude=d["hset"]), 40),
    "decomposition_sweep": (lambda d, c: SW.decomposition_sweep(d["clf"], clusters(d), 2, mode="keep", top=4, chunk_rows=c, support=True,
                                                                pair_support=True), 40),
    "grow_step": (lambda d, c: SW.grow_step(d["clf"], beam(d), d["lo"], d["lo"] + 12, chunk_rows=c), 20),
    "kway_expected": (lambda d, c: expected_dict(EX.kway_expected(d["clf"], [(d["lo"], d["lo"] + 12), (d["lo"] + 12, d["lo"] + 24)], K3, GAP,
                                                                  chunk_rows=c)), 100),
    "kway_enriched_sweep_cached": (lambda d, c: enriched(d, c), 100),
    "kway_enriched_sweep_twice": (lambda d, c: enriched(d, c, cache_rows=0), 100),
}

EXCLUDING = {"kway_sweep_exclude", "kway_map", "region_sweep", "region_sweep_per_leading", "region_map", "kway_enriched_sweep_cached",
             "kway_enriched_sweep_twice"}

FORWARD = ("row_count_kernel", "row_scan_kernel", "row_fill_kernel", "tile_compact_kernel", "tile_pack_kernel", "zero_f32_kernel",
           "front_fwd3_kernel", "fused_fwd32_kernel")                   # one model(x) of up to 8 columns on the pinned route: each once


def counts(forwards, **others):
    return {**{kernel: forwards for kernel in FORWARD}, **{f"{name}_kernel": n for name, n in others.items()}}


TOPK = dict(topk_init=1, topk_keys=3, topk_merge=3, topk_commit=3, topk_read=1)
SEGTOPK = dict(segtopk_init=1, segtopk_keys=3, segtopk_merge=3, segtopk_commit=3, segtopk_read=1)
PAIRMAP = dict(pairmap_init=1, pairmap_update=3, pairmap_read=4)
GAPSTATS = dict(gap_stats_init=1, gap_stats_update=3, gap_stats_read=1)

# {kernel: launches} of the three-chunk call, recorded before the loop was shared (the rows kernel: once per chunk, and once more for the
# winners' rows)
LAUNCHES = {
    "kway_sweep": counts(3, kway_rows=4, **TOPK),
    "kway_sweep_exclude": counts(3, kway_rows=4, hashset_contains=3, **TOPK),
    "kway_map": counts(3, kway_rows=3, hashset_contains=3, **PAIRMAP),
    "region_sweep": counts(3, kway_region_rows=4, hashset_contains=3, **TOPK),
    "region_sweep_per_leading": counts(3, kway_region_rows=4, hashset_contains=3, **SEGTOPK),
    "region_map": counts(3, kway_region_rows=3, hashset_contains=3, **PAIRMAP),
    # two size groups of three chunks each; per group the winners' rows and their chosen ids
    "decomposition_sweep": counts(6, cluster_subset_rows=10, segtopk_init=2, segtopk_keys=6, segtopk_merge=6, segtopk_commit=6, segtopk_read=2,
                                  subset_support_init=2, subset_support_update=6, subset_support_read=2,
                                  subset_pair_init=2, subset_pair_update=6, subset_pair_read=2),
    "grow_step": counts(3, grow_twins=1, kway_complete_rows=4, grow_twin_flags=3, **SEGTOPK),
    "kway_expected": counts(6, kway_rows=6, gap_stats_init=1, gap_stats_update=6, gap_stats_read=1),      # two regions of three chunks
    # the expectation's pass, the ranking pass, the winners' rows; gap_enrich once more for the winners' strata
    "kway_enriched_sweep_cached": counts(3, kway_rows=7, gap_enrich=4, hashset_contains=3, **GAPSTATS, **TOPK),
    "kway_enriched_sweep_twice": counts(7, kway_rows=7, gap_enrich=4, hashset_contains=3, **GAPSTATS, **TOPK),
}


def same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for key, v in a.items():
        if isinstance(v, torch.Tensor):
            assert v.dtype == b[key].dtype and torch.equal(v, b[key]), key
        else:
            assert isinstance(v, int) and v == b[key], key


@pytest.mark.parametrize("name", sorted(CASES))
def test_three_chunks_equal_one_and_launch_what_they_launched(d64, name):
    run, chunk_rows = CASES[name]
    d64["clf"]._runtime()                                                # (packing the model's parameters is not the sweep's doing)
    whole = run(d64, 1 << 20)
    with _lib.launch_log() as log:
        cut = run(d64, chunk_rows)
    same(cut, whole)
    assert cut.get("n_candidates", 1) > 0 and cut.get("n_rows", 1) > 0
    if name in EXCLUDING:
        assert cut["n_excluded"] > 0
    assert {k: v for k, v in log.counts.items() if v} == LAUNCHES[name]


def test_the_cache_saves_one_pass_of_forwards(d64):
    """With the cache the enriched sweep's forward runs for the expectation's pass only: the uncached run launches every kernel of the
    forward once more per chunk and once for the winners' logits; the two results are equal."""
    cached, twice = enriched(d64, 100), enriched(d64, 100, cache_rows=0)
    same(cached, twice)
    with _lib.launch_log() as log, torch.no_grad(), _lib.option("disable_small_batch"):
        d64["clf"](SW.kway_rows(d64["lo"], 12, K3, GAP, count=100))
    forward = {k: v for k, v in log.counts.items() if v and k != "kway_rows_kernel"}
    assert forward
    one, two = LAUNCHES["kway_enriched_sweep_cached"], LAUNCHES["kway_enriched_sweep_twice"]
    for kernel, per_call in forward.items():
        assert one[kernel] == 3 * per_call and two[kernel] == (2 * 3 + 1) * per_call, kernel
    assert {k: v for k, v in two.items() if k not in forward} == {k: v for k, v in one.items() if k not in forward}
