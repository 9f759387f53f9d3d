"""The two associations of a head's contribution to `dyn` in the fused embed_dim-64 forward (matcha_amd/csrc/fused_fwd32.hip), restated in numpy
with the bf16x3 split of tests/test_cpu_bf16x3.py and compared with fp64:

  M z      dyn += M_h (sum_j w_j x_hat_j)          fused_fwd32h_kernel (and fused_fwd32_kernel before the y tile): z in an f32 fma chain over the keys,
                                                   then the six-plane product accumulated onto dyn
  sum p y  dyn += sum_j w_j (M_h x_hat_j)          fused_fwd32_kernel: y_j = M_h x_hat_j as the six-plane product into a ZERO accumulator (the value
                                                   table's rows, node_r_kernel's V role), then an f32 fma chain over the keys onto dyn

w_j = p_ij for the k real keys, in order, then n_pad p_i,pad for the padding token's row; the weights sum to 1.  Inputs: LayerNorm-normalised rows,
M with entries of 1 / sqrt(64) standard deviation, a standard-normal starting `dyn`, p drawn on the simplex (and one case with all weight on one
key), k = 2..8, n_pad = 0..6.

The error is counted in units of f32 epsilon (2^-23) of the element's scale S = |dyn| + sum_j w_j sum_f |M_ef| |x_hat_jf|.  On these inputs the
restatement of the M z form -- the form the kernels have used so far -- reaches 1.33 such units at its worst element (1.01 .. 1.33 over k = 2..8,
mean 0.12 .. 0.14): the bound for BOTH forms is BOUND = 1.5 units, that figure rounded up.  The sum p y form measures 0.58 .. 0.83 at its worst
element, mean 0.08 .. 0.09: its products round against a zero accumulator instead of against `dyn`, so it sits below the form it replaces."""
import numpy as np
import pytest

from tests.test_cpu_bf16x3 import split3

EPS = 2.0 ** -23
BOUND = 1.5


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _mfma_chain(acc, m, x):
    """acc[e] += sum_f m[e, f] x[f] the way W32_CHAIN runs it: per 16-slot chunk the six plane products, smallest first, each ONE MFMA -- sixteen exact
    bf16 x bf16 products summed (float64 here: the order inside the instruction is not specified) and added to the f32 accumulator."""
    mh, mm, ml = split3(m)
    xh, xm, xl = split3(x)
    acc = np.asarray(acc, np.float32).copy()
    for c in range(0, 64, 16):
        s = slice(c, c + 16)
        for a, b in ((ml, xh), (mh, xl), (mm, xm), (mm, xh), (mh, xm), (mh, xh)):
            acc = _f32(acc.astype(np.float64) + (a[:, s].astype(np.float64) * b[None, s].astype(np.float64)).sum(1))
    return acc


def _fma_rows(acc, wts, rows):
    """acc += w_j rows_j, one f32 fma per element and key, keys in order"""
    acc = np.asarray(acc, np.float32).copy()
    for wj, rj in zip(wts, rows):
        acc = _f32(acc.astype(np.float64) + np.float64(np.float32(wj)) * rj.astype(np.float64))
    return acc


def _case(rng, k, n_pad, one_hot=False):
    x = rng.standard_normal((k + 1, 64))
    x = _f32((x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5))       # rows k: the padding token's
    m = _f32(rng.standard_normal((64, 64)) / 8.0)
    dyn = _f32(rng.standard_normal(64))
    slots = k + n_pad
    p = np.zeros(slots) if one_hot else rng.dirichlet(np.full(slots, 0.7))
    if one_hot:
        p[rng.integers(0, slots)] = 1.0
    p = _f32(p)
    p_pad = p[k] if n_pad else np.float32(0.0)             # the padding slots share one score, so one probability
    wts = list(p[:k]) + [np.float32(np.float32(n_pad) * p_pad)]
    return x, m, dyn, wts


def _errors(x, m, dyn, wts):
    w64 = np.array([np.float64(w) for w in wts])
    z64 = (w64[:, None] * x.astype(np.float64)).sum(0)
    exact = dyn.astype(np.float64) + m.astype(np.float64) @ z64
    scale = np.abs(dyn.astype(np.float64)) + np.abs(m.astype(np.float64)) @ (w64[:, None] * np.abs(x.astype(np.float64))).sum(0)
    mz = _mfma_chain(dyn, m, _fma_rows(np.zeros(64, np.float32), wts, x))
    y = [_mfma_chain(np.zeros(64, np.float32), m, xj) for xj in x]
    py = _fma_rows(dyn, wts, y)
    unit = EPS * scale
    return np.abs(mz - exact) / unit, np.abs(py - exact) / unit


@pytest.mark.parametrize("k", range(2, 9))
def test_both_associations_hold_the_same_multiple_of_epsilon(k):
    rng = np.random.default_rng(150 + k)
    worst = [0.0, 0.0]
    mean = [[], []]
    for n_pad in range(0, 7):
        for rep in range(6):
            e_mz, e_py = _errors(*_case(rng, k, n_pad, one_hot=rep == 5))
            for i, e in enumerate((e_mz, e_py)):
                worst[i] = max(worst[i], float(e.max()))
                mean[i].append(float(e.mean()))
    print(f"k = {k}: M z worst {worst[0]:.3f} mean {np.mean(mean[0]):.3f} | sum p y worst {worst[1]:.3f} mean {np.mean(mean[1]):.3f}  (units of eps x scale)")
    assert worst[0] <= BOUND, ("M z", k, worst[0])
    assert worst[1] <= BOUND, ("sum p y", k, worst[1])


def test_the_associations_differ_in_rounding_only():
    """Same function: the two results differ by no more than the two bounds together -- and do differ (which is why every path of the single-wave
    kernel had to change formulation together to stay bitwise equal to the others)."""
    rng = np.random.default_rng(149)
    differ = 0
    for k in range(2, 9):
        x, m, dyn, wts = _case(rng, k, 8 - k if k < 8 else 0)
        mz = _mfma_chain(dyn, m, _fma_rows(np.zeros(64, np.float32), wts, x))
        py = _fma_rows(dyn, wts, [_mfma_chain(np.zeros(64, np.float32), m, xj) for xj in x])
        w64 = np.array([np.float64(w) for w in wts])
        scale = np.abs(dyn.astype(np.float64)) + np.abs(m.astype(np.float64)) @ (w64[:, None] * np.abs(x.astype(np.float64))).sum(0)
        assert (np.abs(mz.astype(np.float64) - py.astype(np.float64)) <= 2 * BOUND * EPS * scale).all()
        differ += int((mz != py).any())
    assert differ == 7
