"""The per-pair support planes restated in numpy: the twin of csrc/sweep_support.hip's subset_pair_update_kernel.  No GPU, no
torch; tests/test_cpu_pair_support.py and tests/test_hip_pair_support.py both check against it.

The rule.  Row i of an update has the global rank g0 + i, hence cluster a = g // C(S, m) and the choice of rank g % C(S, m)
(tests/subsets_ref.py's choices).  A skipped row does nothing, a row whose value is NaN, negative or > vmax counts as rejected, every
other row adds quantum(v) and 1 to the cell of every pair i < j of its chosen positions.  A plane is [A, P], P = S (S - 1) / 2: the upper
triangle row-major, pair (i, j) in column i (2 S - i - 1) / 2 + (j - i - 1)."""
import itertools

import numpy as np

from tests import subsets_ref as SR


def pair_cell(S, i, j):
    """The packed column of positions i < j."""
    return i * (2 * S - i - 1) // 2 + (j - i - 1)


def pair_cells(S, m):
    """int64 [C(S, m), C(m, 2)]: the packed columns every choice adds to, in rank order."""
    ch = np.asarray(SR.choices(S, m), dtype=np.int64).reshape(-1, m)
    ci, cj = np.asarray(list(itertools.combinations(range(m), 2)), dtype=np.int64).T
    return pair_cell(S, ch[:, ci], ch[:, cj])


def unpack(S, plane):
    """[A, P] -> the symmetric [A, S, S] with a zero diagonal."""
    plane = np.asarray(plane)
    i, j = np.triu_indices(S, 1)                                         # row-major, the packed order
    assert np.array_equal(pair_cell(S, i, j), np.arange(S * (S - 1) // 2))
    full = np.zeros((plane.shape[0], S, S), dtype=plane.dtype)
    full[:, i, j] = plane
    full[:, j, i] = plane
    return full


def pair_support(A, S, m, values, skip, g0, vmax=1.0, state=None):
    """(sum int64 [A, P], count int64 [A, P], [n_rows, n_rejected]) after one update of rows g0 .. g0 + len(values) - 1 on top of
    ``state`` (the same triple, or None).  The sums wrap modulo 2^64 as the kernel's do."""
    P = S * (S - 1) // 2
    if state is None:
        state = (np.zeros((A, P), dtype=np.int64), np.zeros((A, P), dtype=np.int64), [0, 0])
    total, cnt, counters = state
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    n = len(v)
    skipped = np.zeros(n, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        okv = (v >= 0) & (v <= np.float32(vmax))                         # False for NaN
    live = ~skipped & okv
    counters[0] += int(live.sum())
    counters[1] += int((~skipped & ~okv).sum())
    cells = pair_cells(S, m)
    cm = len(cells)
    g = g0 + np.flatnonzero(live)
    assert n == 0 or (g0 >= 0 and g0 + n <= A * cm)
    q = np.fromiter((SR.quantum(x) for x in v[live]), dtype=np.int64, count=len(g))
    at = (g // cm)[:, None] * P + cells[g % cm]                          # [rows, C(m, 2)] flat cells
    with np.errstate(over="ignore"):
        np.add.at(total.reshape(-1), at.reshape(-1), np.repeat(q, cells.shape[1]))
    np.add.at(cnt.reshape(-1), at.reshape(-1), 1)
    return total, cnt, counters
