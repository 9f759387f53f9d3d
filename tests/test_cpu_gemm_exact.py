"""The method of tests/test_hip_gemm_exact.py, checked without a GPU.

The GPU tests hold matcha_gemm to bit-exact results on inputs whose products and partial sums are exactly representable.  This file
shows, on a numpy emulation of the wide kernels' arithmetic (three bf16 planes per operand, six plane products per 16-slot chunk,
f32 accumulation: tests/test_cpu_bf16x3.py), that

* the correct six-product scheme returns the exact result on every kind of input the GPU tests use;
* dropping any ONE of the six plane products is a bit mismatch on at least one of the three selection inputs;
* the graded random criterion of the GPU tests passes the correct scheme and rejects every scheme with a plane dropped;
* every shape of the GPU tests reaches the kernel path it is listed under, by the dispatch rule restated in tests/gemm_ref.py;
* the float64 reference's epilogue is the one plain torch ops give, and its dropout mask is oracle/rng.py's."""
import numpy as np
import pytest
import torch

from oracle import rng as R
from tests import gemm_ref as G
from tests.test_cpu_bf16x3 import split3

TERMS = ("AlBh", "AhBl", "AmBm", "AmBh", "AhBm", "AhBh")       # gemm_wide.hip::mma6, smallest first


def mm_bf16x3(A, Bnk, drop=None):
    """A [M,K] . Bnk [N,K]^T as the wide kernels compute it: per 16-slot chunk the six plane products in mma6's order, each one MFMA =
    16 exact bf16 x bf16 products per output added to the f32 accumulator (float64 inside the instruction, rounded once).  ``drop``
    names one term to leave out (a wrong kernel)."""
    A, Bnk = np.asarray(A, np.float32), np.asarray(Bnk, np.float32)
    K = A.shape[1]
    pad = (-K) % 16
    if pad:
        A = np.pad(A, ((0, 0), (0, pad)))
        Bnk = np.pad(Bnk, ((0, 0), (0, pad)))
    ah, am, al = (x.astype(np.float64) for x in split3(A))
    bh, bm, bl = (x.astype(np.float64) for x in split3(Bnk))
    planes = dict(AlBh=(al, bh), AhBl=(ah, bl), AmBm=(am, bm), AmBh=(am, bh), AhBm=(ah, bm), AhBh=(ah, bh))
    acc = np.zeros((A.shape[0], Bnk.shape[0]), np.float32)
    for c in range(0, A.shape[1], 16):
        for t in TERMS:
            if t == drop:
                continue
            x, y = planes[t]
            acc = (acc.astype(np.float64) + x[:, c:c + 16] @ y[:, c:c + 16].T).astype(np.float32)
    return acc


def _exact_ref(A, Bnk):
    ref = A.double() @ Bnk.double().t()
    G.assert_f32_exact(ref, "product")
    return ref.float().numpy()


M_, N_, K_ = 96, 80, 64


def _selection(kind):
    return G.SELECTIONS[kind](G.NT, M_, N_, K_, G.gen(11 + ord(kind)))


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_six_products_are_exact_on_selection_inputs(kind):
    A, Bnk = _selection(kind)
    ref = _exact_ref(A, Bnk)
    assert np.count_nonzero(ref) >= ref.size // 8          # the comparison is not of zeros
    assert np.array_equal(mm_bf16x3(A.numpy(), Bnk.numpy()), ref)


@pytest.mark.parametrize("K", [5, 64, 250, 2048])
def test_six_products_are_exact_on_dense_integers(K):
    g = G.gen(K)
    A, Bnk = G.ints(g, (M_, K), 31), G.ints(g, (N_, K), 31)
    assert G.dense_int_bound(K, 31) < 2 ** 24
    assert np.array_equal(mm_bf16x3(A.numpy(), Bnk.numpy()), _exact_ref(A, Bnk))


def test_selection_tn_input_is_exact_and_spread_over_the_rows():
    A, B = G.selection_tn(70, 130, 1000, G.gen(3))
    c, _ = G.tn_ref64(A, B, exact=True)
    rows = B.abs().sum(1).nonzero().flatten()
    assert len(rows) == 130 and int(rows.min()) < 64 and int(rows.max()) >= 1000 - 64          # first and last partition of 64 rows
    assert np.array_equal(mm_bf16x3(A.t().contiguous().numpy(), B.t().contiguous().numpy()), c.float().numpy())


@pytest.mark.parametrize("term", TERMS)
def test_a_dropped_plane_product_is_a_bit_mismatch_on_a_selection_input(term):
    caught = []
    for kind in "abc":
        A, Bnk = _selection(kind)
        if not np.array_equal(mm_bf16x3(A.numpy(), Bnk.numpy(), drop=term), _exact_ref(A, Bnk)):
            caught.append(kind)
    assert caught, f"dropping {term} passes every selection input"
    # which input sees which term: (a) B = 2^e needs every plane of A against Bh; (b) the mirror image; (c) 12-bit values need h and m of both
    want = dict(AlBh="a", AhBl="b", AmBm="c")
    if term in want:
        assert want[term] in caught


GRADE_K = sorted({K for _, _, K in G.GRADED_SHAPES})


@pytest.mark.parametrize("K", GRADE_K)
def test_graded_criterion_passes_six_products_and_rejects_every_dropped_plane(K):
    """e(X) = rms(X - R64) / rms(R64) <= 4 * max(e(R32), 2^-23) on randn x 0.2 randn, at the four K of the GPU tests: the correct scheme is
    inside, every scheme with one plane product dropped is outside."""
    assert GRADE_K == [64, 192, 256, 2048]
    A, W = G.graded_inputs(256, 128, K)
    bound, ref = G.graded_bound(A, W)
    e6 = G.rel_rms(torch.from_numpy(mm_bf16x3(A.numpy(), W.numpy())), ref)
    print(f"K={K}: bound {bound:.3e}, six products {e6:.3e}")
    assert e6 <= bound
    for term in TERMS:
        e = G.rel_rms(torch.from_numpy(mm_bf16x3(A.numpy(), W.numpy(), drop=term)), ref)
        print(f"   {term} dropped: {e:.3e}")
        assert e > bound, (term, e, bound)


# ---- the dispatch rule: every shape of the GPU tests reaches the path it is listed under ----------------------------------------
def _expected(case):
    M, N, K = case["shape"]
    mis = case["misalign"]
    return G.expected_kernel(case["op"], M, N, K, wide_disabled=case["wide_disabled"], a_aligned=mis != "A", b_aligned=mis != "B",
                             out_aligned=mis not in ("C", "bias"))


@pytest.mark.parametrize("i", range(len(G.PRODUCT_CASES)))
def test_product_case_reaches_its_path(i):
    case = G.PRODUCT_CASES[i]
    path = _expected(case)
    for k, v in case["want"].items():
        assert getattr(path, k) == v, (case, path)


def test_the_listed_shapes_cover_every_branch_of_the_rule():
    paths = [(c, _expected(c)) for c in G.PRODUCT_CASES]
    seen = {(p.kernel, p.bk, p.vec, min(p.ntpb or 1, 2)) for _, p in paths}
    for want in [("gemm_rm_kernel", None, True, 1), ("gemm_rm_kernel", None, False, 1), ("gemm_lds_kernel", 64, None, 1),
                 ("gemm_lds_kernel", 64, None, 2), ("gemm_lds_kernel", 32, None, 1), ("gemm_wide_kernel", None, None, 1),
                 ("gemm_wide_kernel", None, None, 2)]:
        assert want in seen, want
    cd = G.cdiv
    # lds kernel, ntpb = 8 at nine column tiles: two column groups, the second holds ONE tile with 8 live columns; partial k chunk
    M, N, K = 16300, 520, 40
    assert cd(N, 64) == 9 and cd(cd(N, 64), 8) == 2 and N - 8 * 64 == 8 and cd(M, 128) * 2 >= 256 and cd(M - 1, 128) * 2 < 256 + 2 and K % 64 != 0
    assert G.expected_kernel(G.NT, 16256, 520, 40).ntpb == 1                   # one row tile fewer: back to one column tile per workgroup
    # lds kernel, ntpb = 2 at two column tiles
    assert G.expected_kernel(G.NT, 32700, 128, 64, wide_disabled=True).ntpb == 2 and G.expected_kernel(G.NT, 32640, 128, 64, wide_disabled=True).ntpb == 1
    # the small lds shapes: partial last column tile and partial (only) k chunk; BK = 32 with a partial LAST chunk
    assert 72 % 64 != 0 and 40 % 64 != 0 and 68 % 32 == 4 and 252 % 32 == 28 and 24 % 64 != 0
    # wide kernel at ntpb = 2: 15 x 275 = 4 125 tiles, 2 063 workgroups in 2 064 launched (nwg % 8 != 0: one launched workgroup returns
    # early), the last workgroup is short (one tile), the last row tile has one live row
    M, N, K = 35073, 1920, 64
    p = G.expected_kernel(G.NT, M, N, K)
    nx, ny = N // 128, cd(M, 128)
    assert (nx, ny, nx * ny) == (15, 275, 4125) and p.ntpb == 2 and p.nwg == 2063 and p.launched == 2064 and p.nwg % 8 != 0
    assert nx * ny - (p.nwg - 1) * p.ntpb == 1 and M - (ny - 1) * 128 == 1 and K // 32 == 2
    assert nx % p.ntpb == 1                                                   # a workgroup's two tiles also straddle row tiles
    # the wide kernel is not eligible below K = 64 or off its tile multiples, and falls back when an epilogue operand is misaligned
    assert G.expected_kernel(G.NT, 129, 128, 64, out_aligned=False).kernel == "gemm_lds_kernel"
    assert G.expected_kernel(G.NT, 129, 128, 64).kernel == "gemm_wide_kernel" and G.expected_kernel(G.NT, 129, 128, 32).kernel == "gemm_lds_kernel"


@pytest.mark.parametrize("i", range(len(G.TN_CASES)))
def test_tn_case_reaches_its_path(i):
    (M, N, R_), gather, want = G.TN_CASES[i]
    path = G.expected_kernel(G.TN, M, N, R_, gather=gather)
    for k, v in want.items():
        assert getattr(path, k) == v, (G.TN_CASES[i], path)
    assert path.P * path.rows_per_block >= R_ > (path.P - 1) * path.rows_per_block          # the partitions tile the rows, none empty


def test_the_other_case_lists_reach_their_kernels():
    for op in (G.NT, G.NN):
        kernels = set()
        for (M, N, K), wd, kernel in G.EPILOGUE_SHAPES[op] + G.LARGE_EPILOGUE_SHAPES:
            assert G.expected_kernel(op, M, N, K, wide_disabled=wd).kernel == kernel
            kernels.add((kernel, G.expected_kernel(op, M, N, K, wide_disabled=wd).bk))
        assert kernels == {("gemm_rm_kernel", None), ("gemm_lds_kernel", 64), ("gemm_lds_kernel", 32), ("gemm_wide_kernel", None)}
        # every instantiation of the switch, and two sets that reach the generic one
        inst = [G.epilogue_instance(op, f) for f in G.EPILOGUE_SETS[op]]
        assert set(inst) == set(G.SPECIALISED[op]) | {-1} and inst.count(-1) == 2
    assert G.epilogue_instance(G.NT, G.LARGE_EPILOGUE_FLAGS[G.NT]) >= 0 and G.epilogue_instance(G.NN, G.LARGE_EPILOGUE_FLAGS[G.NN]) >= 0
    for op, (M, N, K), wd, kernel in G.SELECTION_CASES:
        assert G.expected_kernel(op, M, N, K, wide_disabled=wd).kernel == kernel
    for (M, N, R_), kernel in G.SELECTION_TN_CASES:
        assert G.expected_kernel(G.TN, M, N, R_).kernel == kernel
    fam = set()
    for M, N, K in G.GRADED_SHAPES:
        for wd in (False, True):
            p = G.expected_kernel(G.NT, M, N, K, wide_disabled=wd)
            fam.add((p.kernel, p.bk))
        assert G.expected_kernel(G.NT, M, N, K, a_aligned=False).kernel == "gemm_rm_kernel"
    assert fam == {("gemm_lds_kernel", 64), ("gemm_lds_kernel", 32), ("gemm_wide_kernel", None)}


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def test_dropout_mask_in_torch_ops_is_the_oracles():
    for seed, p, shape in [(123456789012345, 0.5, (300, 70)), (75, 0.9, (2000, 64)), (2 ** 63 + 5, 0.3, (17, 1921))]:
        want = torch.from_numpy(R.dropout_mask(seed, R.STREAM_DROP_FC1, p, *shape))
        assert torch.equal(G.dropout_mask_torch(seed, R.STREAM_DROP_FC1, p, *shape), want)
    assert float(G.dropout_mask_torch(1, R.STREAM_DROP_FC1, 0.5, 4, 64).max()) == 2.0          # the keep scale of the exact cases


def test_reference_epilogue_is_what_torch_ops_give():
    M, N, K = 33, 20, 12
    g = G.gen(5)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3
    bias, res, C0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    aux = torch.tanh(torch.randn(M, N, generator=g))
    ids = torch.randint(0, 3, (M,), generator=g)
    seed, p = 4242, 0.3
    mask = torch.from_numpy(R.dropout_mask(seed, R.STREAM_DROP_FC1, p, M, N))
    kw = dict(bias=bias, residual=res, aux=aux, aux_scale=0.7, row_ids=ids, seed=seed, stream=R.STREAM_DROP_FC1, p=p, C0=C0)
    lin = torch.nn.functional.linear(A, W)
    rowm = (ids != 0).float()[:, None]
    want = {
        0: lin,
        G.BIAS | G.TANH: torch.tanh(lin + bias),
        G.BIAS | G.TANH | G.RESIDUAL | G.DROPOUT | G.ROWMASK: (torch.tanh(lin + bias) + res) * mask * rowm,
        G.DROPOUT | G.DTANH: lin * mask * (1 - (aux * 0.7) ** 2),
        G.RESIDUAL | G.ROWMASK: (lin + res) * rowm,
        G.ACCUM: lin + C0,
        G.ALL_FLAGS: (torch.tanh(lin + bias) + res) * mask * rowm * (1 - (aux * 0.7) ** 2) + C0,
    }
    for flags, w in want.items():
        got, dead = G.gemm_ref64(G.NT, A, W, flags, **kw)
        assert float((got - w.double()).abs().max()) <= 1e-5, flags
        got_nn, _ = G.gemm_ref64(G.NN, A, W.t().contiguous(), flags, **kw)
        assert torch.equal(got, got_nn)
        want_dead = torch.zeros(M, N, dtype=torch.bool)
        if flags & G.DROPOUT:
            want_dead |= mask == 0
        if flags & G.ROWMASK:
            want_dead |= (ids == 0)[:, None]
        assert torch.equal(dead, want_dead)
    # order matters and is the kernels': the residual is added AFTER tanh and BEFORE dropout
    got, _ = G.gemm_ref64(G.NT, A, W, G.TANH | G.RESIDUAL | G.DROPOUT, **kw)
    assert float((got - ((torch.tanh(lin) + res) * mask).double()).abs().max()) <= 1e-5
    c, cs = G.tn_ref64(A, res[:, :7], C0=C0[:K, :7], col0=bias[:K])
    assert float((c - (A.t() @ res[:, :7] + C0[:K, :7]).double()).abs().max()) <= 1e-5 and float((cs - (A.sum(0) + bias[:K]).double()).abs().max()) <= 1e-5
    idx = torch.randint(0, M, (50,), generator=g)
    c2, _ = G.tn_ref64(torch.randn(50, 5, generator=g), res, gather=idx)
    assert c2.shape == (5, N)


@pytest.mark.parametrize("op", [G.NT, G.NN])
def test_epilogue_inputs_are_exact_at_every_stage(op):
    """every flag set on every small epilogue shape: no stage of the float64 reference rounds in float32 (TANH sets: up to the exact
    pre-activation, which lies in [-4, 4])"""
    for (M, N, K), _, _ in G.EPILOGUE_SHAPES[op]:
        for flags in G.EPILOGUE_SETS[op]:
            d = G.epilogue_inputs(op, M, N, K, flags)
            A, B = d.pop("A"), d.pop("B")
            d.pop("flags")
            ref, dead = G.gemm_ref64(op, A, B, flags, exact=True, **d)
            if flags & G.TANH:
                pre, _ = G.gemm_ref64(op, A, B, flags & G.BIAS, exact=True, **d)
                assert 2.0 <= float(pre.abs().max()) <= 4.0
                assert float(ref.abs().max()) < 32.0
            else:
                G.assert_f32_exact(ref, "result")
            if flags & (G.DROPOUT | G.ROWMASK):
                assert 0 < int(dead.sum()) < dead.numel()
    # the large shapes' products stay integers below 2^24 as well (dropout doubles, bias / residual add at most 1000)
    for (M, N, K), _, _ in G.LARGE_EPILOGUE_SHAPES:
        assert 2 * (G.dense_int_bound(K, 31) + 1000) < 2 ** 24
    for (M, N, R_), _, _ in G.TN_CASES:
        assert G.dense_int_bound(R_, 31) + 1000 < 2 ** 24
