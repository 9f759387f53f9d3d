"""The value-table form of the merged heads' backward against the dZ form, in fp64 numpy (tests/node_v_ref.py): the identities
fused_bwdh_kernel<ML, true, true> rests on -- d_j = dDyn_i . (M_h x_hat_j), sum_i p_ij dz_i = U_j M_h, dM_h = U^T x_hat + u_pad (x) x_hat_pad,
d x_hat_pad = accK + u_pad M_h -- hold to rounding, and each of the two padding terms is visible wherever a row has a padding key."""
import numpy as np
import pytest

from tests import node_v_ref as R

TOL = 1e-12          # of each output's largest element: fp64 sums of <= 64 x 35 terms of O(1) reordered

CASES = {
    "L5 k2..5": ([2, 3, 4, 5], 5),
    "L5 mixed, two tiles' worth": ([5, 2, 3, 3, 4, 2, 5, 4], 5),
    "L8 k2..8": ([2, 3, 4, 5, 6, 7, 8], 8),
    "L5 every row full": ([5, 5, 5, 5, 5, 5], 5),
    "L8 every row full": ([8, 8, 8], 8),
    "L5 every row k2": ([2] * 15, 5),
    "L8 every row k2": ([2] * 15, 8),
}
PADDED = [n for n, (ks, L) in CASES.items() if any(k < L for k in ks)]


@pytest.mark.parametrize("name", list(CASES))
def test_value_table_form_equals_the_dz_form(name):
    ks, L = CASES[name]
    inp = R.make_inputs(1000 + len(name), ks, L)
    P, pp = R.probabilities(inp)
    for t0, k in inp["edges"]:                               # the rows are probability rows, diagonal 0, padding slots counted n_pad times
        assert np.allclose(P[t0:t0 + k].sum(1) + (L - k) * pp[t0:t0 + k], 1.0, atol=1e-14)
        assert (np.diag(P[t0:t0 + k, :k]) == 0).all()
    a, b = R.backward_v(inp), R.backward_dz(inp)
    assert set(a) == set(b) == {"dx", "dB", "dM", "db", "dbdyn", "dxpad"}
    err, what, errs = R.worst(a, b)
    print(name, {n: f"{e:.1e}" for n, e in errs.items()})
    assert err <= TOL, (name, what, err)
    if all(k == L for k in ks):                              # no padding key anywhere: the padding token gets no gradient at all
        assert float(np.abs(b["dxpad"]).max()) == 0.0 and float(np.abs(a["dxpad"]).max()) == 0.0


@pytest.mark.parametrize("name", PADDED)
def test_each_padding_term_is_seen_when_dropped(name):
    ks, L = CASES[name]
    inp = R.make_inputs(2000 + len(name), ks, L)
    b = R.backward_dz(inp)
    _, _, e1 = R.worst(R.backward_v(inp, drop_rank_one=True), b)
    assert e1["dM"] > 1e-3 and max(v for n, v in e1.items() if n != "dM") <= TOL, e1       # u_pad (x) x_hat_pad belongs to dM_h alone
    _, _, e2 = R.worst(R.backward_v(inp, drop_upad_m=True), b)
    assert e2["dxpad"] > 1e-3 and max(v for n, v in e2.items() if n != "dxpad") <= TOL, e2  # u_pad M_h to the padding token's d x_hat alone


def test_rows_without_padding_cannot_see_the_terms():
    """Why the GPU tests need the k < L batches: with n_pad = 0 everywhere both wrong variants pass."""
    ks, L = CASES["L5 every row full"]
    inp = R.make_inputs(3000, ks, L)
    b = R.backward_dz(inp)
    assert R.worst(R.backward_v(inp, drop_rank_one=True, drop_upad_m=True), b)[0] <= TOL
