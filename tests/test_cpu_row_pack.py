"""The packed row order of the ragged plan (tests/row_pack_ref.py: the NumPy twin of ragged.hip's schedule and destinations, with the greedy
half-tile packer on top), checked without a GPU: it is a permutation, every hyperedge lies whole in one half tile, every all-padding row is
covered once, the schedule is a function of the class counts alone, and on the benchmark's row sizes the half tiles come within 1 % of
ceil(tokens / 31) where the batch order gives 5.5 % more."""
import numpy as np
import pytest

from tests import row_pack_ref as R


def _rows(k, L, rng, pads_inside=False):
    """A batch [B, L] whose row b holds k[b] ids in 1 .. 150."""
    k = np.asarray(k)
    x = np.zeros((len(k), L), np.int64)
    ids = rng.integers(1, 151, size=x.shape)
    x[np.arange(L)[None, :] < k[:, None]] = 1
    x *= ids
    if pads_inside:
        x = np.take_along_axis(x, np.argsort(rng.random(x.shape), axis=1), axis=1)
    return x


def _check(x, packed=True):
    B, L = x.shape
    p = R.plan(x, 150, packed=packed)
    k = (x != 0).sum(1)
    src, off = p["row_src"].astype(np.int64), p["row_off"].astype(np.int64)
    assert np.array_equal(np.sort(src), np.arange(B))                           # a permutation of the batch's rows
    assert (np.diff(off) == k[src]).all() and off[0] == 0 and off[B] == k.sum() == p["tokens"]      # monotone, each row its own k tokens
    # the tokens of plan row b' are batch row src[b']'s, in the row's order, with the ORIGINAL slots
    slot = p["tok_slot"][:p["tokens"]].astype(np.int64)
    assert np.array_equal(slot // L, np.repeat(src, k[src]))
    assert np.array_equal(p["tok_id"][:p["tokens"]], x.reshape(-1)[slot])
    assert (np.diff(slot)[np.diff(slot // L) == 0] > 0).all()
    assert np.array_equal(p["tok_pos"][:p["tokens"]] >> 8, np.repeat(k[src], k[src]))
    assert p["tok_slot"][p["tokens"]] == B * L and not p["tok_key"][p["tokens"]:].any()
    # half tiles: whole hyperedges, <= 31 tokens, every row (the all-padding ones too) in exactly one, the token stream covered once in order
    t = p["half_meta"].astype(np.int64)
    assert (t[:, 1] <= R.HALF_TOK).all() and (t[:, 3] >= 1).all()
    assert np.array_equal(t[:, 2], np.concatenate([[0], np.cumsum(t[:, 3])[:-1]])) and t[:, 3].sum() == B
    assert np.array_equal(t[:, 0], off[t[:, 2]]) and np.array_equal(t[:, 0] + t[:, 1], off[t[:, 2] + t[:, 3]])
    # the planning superblocks the packer works in hold no more tiles than the workspace reserves for one, and the lists fit
    assert len(t) <= -(-(B * L + 1) // (32 - L)) + len(p["sb_first"]) - 1
    sb = np.searchsorted(p["sb_first"][:-1][p["sb_first"][:-1] < B], t[:, 2], side="right")
    assert np.bincount(sb).max() <= -(-(R.SUPER_TOK + L) // (32 - L)) + 2
    return p


def _bench_k(B=65536, ks=(2, 3, 4, 5), seed=2):
    """The benchmark's row sizes: B / 4 positives with k uniform in ks, then three negatives of each positive's size."""
    kpos = np.random.default_rng(seed).choice(ks, size=B // 4)
    return np.concatenate([kpos, np.repeat(kpos, 3)])


def test_bench_sizes_fill_the_half_tiles():
    rng = np.random.default_rng(3)
    x = _rows(_bench_k(), 5, rng)
    new, old = _check(x), _check(x, packed=False)
    floor = -(-new["tokens"] // R.HALF_TOK)
    print(f"tokens {new['tokens']}  ceil(Tr/31) {floor}  batch order {old['halves']}  packed {new['halves']}  phases {len(new['phases'])}")
    assert new["halves"] <= 1.01 * floor
    assert old["halves"] >= 1.04 * floor                                          # what the order is there to remove
    assert len(new["phases"]) <= R.MAX_PHASES


def test_bench_sizes_k_up_to_8():
    rng = np.random.default_rng(4)
    x = _rows(_bench_k(16384, (2, 3, 4, 5, 6, 7, 8), 5), 8, rng)
    new, old = _check(x), _check(x, packed=False)
    floor = -(-new["tokens"] // R.HALF_TOK)
    print(f"tokens {new['tokens']}  ceil(Tr/31) {floor}  batch order {old['halves']}  packed {new['halves']}  phases {len(new['phases'])}")
    assert new["halves"] <= 1.02 * floor and new["halves"] < old["halves"]


@pytest.mark.parametrize("L", [2, 5, 8])
@pytest.mark.parametrize("B", [1, 2, 7, 255, 256, 257, 3100])
def test_sweep(B, L):
    rng = np.random.default_rng(100 * B + L)
    k = rng.integers(0, L + 1, size=B)
    for pads_inside in (False, True):
        x = _rows(k, L, rng, pads_inside)
        new, old = _check(x), _check(x, packed=False)
        assert new["halves"] <= old["halves"] + 1, (B, L, new["halves"], old["halves"])
        again = R.plan(x, 150)
        assert again["phases"] == new["phases"] and all(np.array_equal(again[n], new[n]) for n in ("row_src", "row_off", "tok_slot", "half_meta"))
        # the schedule depends on the class counts alone: the same rows in another batch order give the same phases
        assert R.schedule(np.bincount(k[rng.permutation(B)], minlength=R.NCLS)) == new["phases"]


@pytest.mark.parametrize("L", [2, 5, 8])
def test_single_class_batches_pack_as_today(L):
    rng = np.random.default_rng(7)
    for k in range(1, L + 1):
        x = _rows(np.full(3100, k), L, rng)
        new, old = _check(x), _check(x, packed=False)
        assert new["halves"] == old["halves"], (L, k)
        assert np.array_equal(new["row_src"], np.arange(3100)) and np.array_equal(new["row_off"], old["row_off"])


def test_all_padding_rows_are_covered_once():
    rng = np.random.default_rng(8)
    x = np.zeros((700, 5), np.int64)
    p = _check(x)
    assert p["tokens"] == 0 and p["halves"] == 1 and p["half_meta"][0].tolist() == [0, 0, 0, 700]
    k = rng.integers(2, 6, size=3072)
    k[200:330] = 0
    k[rng.choice(3072, size=150, replace=False)] = 0
    p = _check(_rows(k, 5, rng, pads_inside=True))
    n0 = int((k == 0).sum())
    # spread over the first phase's tiles, not hung on one
    assert p["half_meta"][:, 3].max() < n0 // 4
    x = np.zeros((3072, 5), np.int64)
    x[1234, :2] = (17, 99)                                                       # one hyperedge of two nodes among all-padding rows
    p = _check(x)
    assert p["halves"] == 1 and p["tokens"] == 2


def test_recipes_hold_31_tokens_while_the_classes_allow():
    for n in ([0, 0, 16384, 16384, 16384, 16384, 0, 0, 0], [5, 40, 1000, 10, 7, 900, 3, 300, 2000], [0, 1 << 28, 0, 0, 0, 0, 0, 0, 1 << 27]):
        ph = R.schedule(n)
        assert 1 <= len(ph) <= R.MAX_PHASES
        assert [sum(p["m"] * p["a"][c] for p in ph) for c in range(R.NCLS)] == list(n)
        for p in ph[:-1]:
            assert p["toks"] <= R.HALF_TOK and p["m"] >= 1
        assert ph[0]["toks"] == R.HALF_TOK
