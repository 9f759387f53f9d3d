"""The multi-region sweep's candidates by brute force: the cases of tests/golden/g18_regions_tiny.npz and the itertools
enumeration that both the fixture's generator and the tests use -- per-part combinations under the gap rule, then their product."""
import itertools

import numpy as np

# (parts as (chromosome, first bin, one past the last bin, m), min_gap) on the tiny layout (4 chromosomes of 16 bins); the windows of cases
# 1 to 3 are the moved ones (tests/golden/make_golden_regions.py says why)
CASES = [
    ([(0, 0, 16, 1), (2, 0, 16, 2)], 1),                                  # 1 920
    ([(0, 0, 8, 1), (1, 0, 8, 1), (3, 8, 16, 2)], 2),                      # 1 344
    ([(2, 0, 6, 2), (2, 6, 16, 2)], 3),                                   # 168, some invalid at the boundary of the two windows
    ([(0, 0, 8, 2), (2, 6, 12, 1), (3, 8, 16, 2)], 2),                    # 2 646, k = 5
]


def case_parts(case, chrom_range):
    """[(lo, hi, m)] in node ids."""
    return [(int(chrom_range[c][0]) + a, int(chrom_range[c][0]) + b, m) for c, a, b, m in case]


def candidates(parts, min_gap, width=None):
    """(rows int64 [T, width], valid bool [T]) in rank order; a row is valid iff all its adjacent differences are >= min_gap."""
    per = [[c for c in itertools.combinations(range(lo, hi), m) if all(b - a >= min_gap for a, b in zip(c, c[1:]))] for lo, hi, m in parts]
    k = sum(m for _, _, m in parts)
    rows = np.asarray([sum(t, ()) for t in itertools.product(*per)], dtype=np.int64).reshape(-1, k)
    valid = (np.diff(rows, axis=1) >= min_gap).all(axis=1)
    return np.pad(rows, ((0, 0), (0, (width or k) - k))), valid
