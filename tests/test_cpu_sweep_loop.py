"""The sweeps' shared loop and the blocks around it (matcha_amd/sweep.py) without a GPU: ``_chunks`` on a stub rows
function, a stub model and a stub ``exclude``; the one decoder against itertools and every public unranker against it; ``_rank_range``
and ``_row_buffers``."""
import itertools

import pytest
import torch

from matcha_amd import sweep as SW

WIDTH = 3


class Rows:
    """Row g is (g + 1, 0, 0); with ``flags`` row g is invalid where flags[g] != 0.  Remembers every call."""

    def __init__(self, flags=None):
        self.flags, self.calls = flags, []

    def __call__(self, g0, count, buf, fbuf):
        self.calls.append((g0, count, buf, fbuf))
        x = buf[:count * WIDTH].view(count, WIDTH)
        x.zero_()
        x[:, 0] = torch.arange(g0 + 1, g0 + count + 1)
        if self.flags is None:
            return x
        fbuf[:count] = self.flags[g0:g0 + count]
        return x, fbuf[:count]


class Known:
    """The rows whose first id is in ``ids``."""

    def __init__(self, ids):
        self.ids = torch.tensor(sorted(ids))

    def contains(self, x):
        return torch.isin(x[:, 0], self.ids)


class Model:
    calls = 0

    def __call__(self, x):
        self.calls += 1
        return x[:, 0].float()


def walk(total, chunk_rows, flags=None, known=None, forward=None, model=None):
    rows = Rows(flags)
    tally = SW._tally("cpu", "n_invalid", "n_excluded")
    buffers = SW._buffers(min(chunk_rows, total), WIDTH, "cpu", flags=flags is not None)
    out = []
    for g0, x, logits, skip, flag in SW._chunks(model or Model(), total, chunk_rows, buffers, rows, known, tally, forward):
        assert (flag is None) == (flags is None) and logits.shape == (x.shape[0],)
        out.append((g0, x.clone(), logits.clone(), None if skip is None else skip.clone()))
    return out, rows, buffers, SW._counted(tally)


@pytest.mark.parametrize("total, chunk_rows, cuts", [(10, 4, [(0, 4), (4, 4), (8, 2)]), (10, 1 << 20, [(0, 10)]), (8, 8, [(0, 8)])])
def test_chunk_boundaries_buffers_and_no_skip(total, chunk_rows, cuts):
    out, rows, (buf, fbuf), counted = walk(total, chunk_rows)
    assert [(g0, count) for g0, count, _, _ in rows.calls] == cuts == [(g0, int(x.shape[0])) for g0, x, _, _ in out]
    assert all(b is buf and f is fbuf for _, _, b, f in rows.calls) and fbuf is None      # one buffer, every chunk
    assert buf.dtype == torch.long and buf.numel() >= min(chunk_rows, total) * WIDTH
    assert all(skip is None for _, _, _, skip in out)                   # no flags, no exclude: the sink gets a null pointer
    assert torch.equal(torch.cat([logits for _, _, logits, _ in out]), torch.arange(1, total + 1).float())
    assert counted == {"n_invalid": 0, "n_excluded": 0}


def test_exclude_without_flags():
    known = Known([2, 3, 9, 40])
    out, _, _, counted = walk(10, 4, known=known)
    skip = torch.cat([s for _, _, _, s in out])
    assert skip.dtype == torch.bool and skip.tolist() == [g + 1 in (2, 3, 9) for g in range(10)]
    assert counted == {"n_invalid": 0, "n_excluded": 3}


@pytest.mark.parametrize("chunk_rows", [1, 3, 10])
def test_flags_and_exclude(chunk_rows):
    flags = torch.tensor([0, 1, 0, 0, 2, 3, 0, 0, 1, 0], dtype=torch.int32)
    known = Known([2, 3, 4, 6, 10])                                      # rows 1, 2, 3, 5, 9: rows 1 and 5 are invalid as well
    invalid, member = flags != 0, torch.tensor([g + 1 in (2, 3, 4, 6, 10) for g in range(10)])
    assert bool((invalid & member).any())
    out, rows, (buf, fbuf), counted = walk(10, chunk_rows, flags=flags, known=known)
    assert fbuf.dtype == torch.int32 and fbuf.numel() >= chunk_rows and all(f is fbuf for _, _, _, f in rows.calls)
    assert torch.equal(torch.cat([s for _, _, _, s in out]), invalid | member)
    assert counted == {"n_invalid": int(invalid.sum()), "n_excluded": int((member & ~invalid).sum())} == {"n_invalid": 4, "n_excluded": 3}


def test_forward_stands_in_for_the_model():
    model, seen = Model(), []

    def forward(g0, x):
        seen.append((g0, int(x.shape[0])))
        return -x[:, 0].float()

    out, _, _, _ = walk(10, 4, forward=forward, model=model)
    assert model.calls == 0 and seen == [(0, 4), (4, 4), (8, 2)]
    assert torch.equal(torch.cat([logits for _, _, logits, _ in out]), -torch.arange(1, 11).float())


# ---- the decoder -------------------------------------------------------------------------------------------------------------------
def subsets(lo, n, f, min_gap):
    return [c for c in itertools.combinations(range(lo, lo + n), f) if all(b - a >= min_gap for a, b in zip(c, c[1:]))]


def test_the_decoder_against_itertools_and_every_unranker_against_it():
    lo, far = 5, 10 ** 6
    for n in range(1, 10):
        for f in range(1, 5):
            for gap in range(1, 4):
                want = subsets(lo, n, f, gap)
                assert len(want) == SW._free_count(n, f, gap)
                got = [SW._subset_unrank(r, lo, n, f, gap) for r in range(len(want))]
                assert got == want, (n, f, gap)                          # lexicographic order, every rank
                for r, row in enumerate(want):
                    if f >= 2:
                        assert SW.kway_unrank(r, lo, n, f, gap) == row
                        assert SW.region_unrank(r, [(lo, lo + n, f)], gap) == (row, True)
                    assert SW.anchored_unrank(r, [far], lo, n, f + 1, gap) == (row + (far,), True)
                    assert SW.completion_unrank(r, [far], lo, n, f, gap) == (row + (far,), True)
    for S in range(2, 10):
        for m in range(2, 5):
            for r, row in enumerate(subsets(1, S, m, 1)):
                assert SW._subset_unrank(r, 1, S, m, 1) == row and SW._choice_unrank(r, S, m) == tuple(v - 1 for v in row)
                assert SW.subset_unrank(r, range(1, S + 1), m) == (row, True)
    for call in (lambda: SW.kway_unrank(10, lo, 5, 2, 1), lambda: SW.kway_unrank(-1, lo, 5, 2, 1), lambda: SW.subset_unrank(6, [1, 2, 3, 4], 2),
                 lambda: SW.completion_unrank(5, [far], lo, 5, 1, 1), lambda: SW.region_unrank(10, [(lo, lo + 5, 2)], 1)):
        with pytest.raises(IndexError):
            call()


# ---- rank range and buffers ----------------------------------------------------------------------------------------------------------
def test_rank_range():
    assert SW._rank_range(100, 0, None, None) == 100 and SW._rank_range(100, 30, None, None) == 70      # the default: everything from rank0
    assert SW._rank_range(100, 30, 70, None) == 70 and SW._rank_range(100, 100, 0, None) == 0 and SW._rank_range(0, 0, None, None) == 0
    for rank0, count in ((-1, 1), (0, -1), (30, 71), (101, None)):
        with pytest.raises(IndexError):
            SW._rank_range(100, rank0, count, None)
    ranks = torch.tensor([5, -3, 1 << 40])                               # a list: its length, whatever rank0 and count say
    assert SW._rank_range(100, -7, None, ranks) == 3 and SW._rank_range(100, 1000, 1000, ranks) == 3


def test_row_buffers():
    cpu = torch.device("cpu")
    x, flag = SW._row_buffers(4, 3, cpu, None, None, "t")
    assert x.shape == (4, 3) and x.dtype == torch.long and flag.shape == (4,) and flag.dtype == torch.int32
    assert SW._row_buffers(4, 3, cpu, None, None, "t", flags=False)[1] is None
    out, flag_out = torch.zeros(20, dtype=torch.long), torch.zeros(6, dtype=torch.int32)
    x, flag = SW._row_buffers(4, 3, cpu, out, flag_out, "t")
    assert x.shape == (4, 3) and flag.shape == (4,) and x.data_ptr() == out.data_ptr() and flag.data_ptr() == flag_out.data_ptr()
    x[:], flag[:] = 7, 7
    assert out.tolist() == [7] * 12 + [0] * 8 and flag_out.tolist() == [7] * 4 + [0] * 2      # views of the given storage
    bad_out = (torch.zeros(20, dtype=torch.int32), torch.zeros(40, dtype=torch.long)[::2], torch.zeros(11, dtype=torch.long),
               torch.zeros(20, dtype=torch.long, device="meta"))
    bad_flag = (torch.zeros(6, dtype=torch.long), torch.zeros(12, dtype=torch.int32)[::2], torch.zeros(3, dtype=torch.int32),
                torch.zeros(6, dtype=torch.int32, device="meta"))       # wrong type, not contiguous, too small, another device
    for bad in bad_out:
        with pytest.raises(ValueError):
            SW._row_buffers(4, 3, cpu, bad, flag_out, "t")
    for bad in bad_flag:
        with pytest.raises(ValueError):
            SW._row_buffers(4, 3, cpu, out, bad, "t")
