"""matcha_gemm held to EXACT results on every kernel path it dispatches to (GPU only, -m gpu).

tests/test_hip_kernels.py pins the GEMM entry at 2e-5 * max|ref| on randn inputs, which a kernel that drops a bf16 plane product, or
loses a factor of 20 in precision some other way, still passes.  Here the inputs are chosen so that every product and every partial
sum, in any summation order, is exactly representable in float32 (tests/gemm_ref.py; tests/test_cpu_gemm_exact.py shows on the CPU
that the method sees each of the six plane products): a correct kernel -- f32 MFMA chain or six bf16 plane products -- must then return
the float64 reference bit for bit, and an index, tail, clamp, prefetch or plane error is a bit mismatch, not 1e-6.  Every case

* asserts the kernel that served it (the launch log against tests/gemm_ref.py::expected_kernel),
* asserts ``float32(ref64) == ref64`` before comparing, and then ``torch.equal``,
* starts from a C full of NaN wherever EPI_ACCUM is off, so an unwritten element cannot pass.

EPI_TANH cases compare with float64 tanh of the exact pre-activation at the suite's 2e-5 absolute; their zero patterns stay exact.
One graded random case per family (rounding on ordinary data) closes the file."""
import ctypes as C

import pytest
import torch

from matcha_amd import _lib
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPN = {G.NT: "NT", G.NN: "NN", G.TN: "TN"}
ON_DEVICE = 1 << 22          # outputs from which inputs and the float64 reference are formed on the device (exact for these inputs)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _off4(t):
    """a copy of t that starts 4 bytes into a fresh buffer: 4-byte but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _dev(t, off=False):
    if t is None:
        return None
    t = t.to(DEV).contiguous()
    assert t.data_ptr() % 16 == 0
    return _off4(t) if off else t


def _run(op, A, B, M, N, K, flags=0, *, bias=None, residual=None, aux=None, aux_scale=1.0, row_ids=None, seed=None, stream=None, p=0.0,
         C0=None, colsum0=None, want_colsum=False, gather=None, misalign=None, wide_disabled=False):
    """One matcha_gemm call under the launch log.  C starts as C0 under EPI_ACCUM, else full of NaN (the column sums likewise).
    Returns (C, colsum or None, {kernel: launches})."""
    lib = _lib.load()
    A, B = _dev(A, misalign == "A"), _dev(B, misalign == "B")
    acc = bool(flags & G.ACCUM)
    out = _dev(C0.to(DEV).clone() if acc else torch.full((M, N), float("nan"), device=DEV), misalign == "C")
    col = None
    if want_colsum:
        col = colsum0.to(DEV).clone() if acc else torch.full((M,), float("nan"), device=DEV)
    keep = [_dev(bias, misalign == "bias"), _dev(residual), _dev(aux), _dev(row_ids), None if seed is None else torch.tensor([seed], dtype=torch.int64, device=DEV),
            _dev(gather)]
    epi = None
    if flags:
        epi = _lib.GemmEpilogue()
        epi.flags = flags
        epi.bias, epi.residual, epi.aux, epi.row_ids, epi.seed = (None if t is None else t.data_ptr() for t in keep[:5])
        epi.stream_id, epi.p_drop, epi.aux_scale = (stream or 0), p, aux_scale
    ws, wsn = None, 0
    if op == G.TN:
        wsn = lib.matcha_gemm_tn_workspace_bytes(M, N, K)
        ws = torch.empty(wsn, dtype=torch.uint8, device=DEV)
    with _lib.option("disable_wide_gemm", 1 if wide_disabled else 0):
        with _lib.launch_log() as log:
            _lib.check(lib.matcha_gemm(op, _lib.ptr(A), _lib.ptr(B), _lib.ptr(out), M, N, K, None if epi is None else C.byref(epi),
                                       _lib.ptr(col), _lib.ptr(keep[5]), _lib.ptr(ws), wsn, _stream()), "matcha_gemm")
    torch.cuda.synchronize()
    return out, col, log.counts


def _where(M, N):
    return DEV if M * N >= ON_DEVICE else "cpu"


def _assert_equal(out, ref64, what=""):
    G.assert_f32_exact(ref64, "reference")
    ref = ref64.float().to(out.device)
    if not torch.equal(out, ref):
        bad = (out != ref) | out.isnan()
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {float(out[tuple(idx)])!r}, "
                             f"want {float(ref[tuple(idx)])!r}")


# ---- dense integers on every path -------------------------------------------------------------------------------------------------
def _case_id(c):
    M, N, K = c["shape"]
    return f"{OPN[c['op']]}-{M}x{N}x{K}" + ("-nowide" if c["wide_disabled"] else "") + (f"-off4{c['misalign']}" if c["misalign"] else "")


@pytest.mark.parametrize("case", G.PRODUCT_CASES, ids=_case_id)
def test_dense_integers_are_exact_on_every_path(case):
    op, (M, N, K), mis = case["op"], case["shape"], case["misalign"]
    path = G.expected_kernel(op, M, N, K, wide_disabled=case["wide_disabled"], a_aligned=mis != "A", b_aligned=mis != "B",
                             out_aligned=mis not in ("C", "bias"))
    assert path.kernel == case["want"]["kernel"]
    dev = _where(M, N)
    g = G.gen(M * 7 + N * 3 + K + op, dev)
    sa, sb = G.operand_shapes(op, M, N, K)
    A, B = G.ints(g, sa, 31), G.ints(g, sb, 31)
    flags, bias = 0, None
    if mis == "bias":
        flags, bias = G.BIAS, G.ints(g, (N,), 1000)
    ref, _ = G.gemm_ref64(op, A, B, flags, bias=bias, exact=True)
    out, _, counts = _run(op, A, B, M, N, K, flags, bias=bias, misalign=mis, wide_disabled=case["wide_disabled"])
    assert counts == {path.kernel: 1}, counts
    _assert_equal(out if dev == DEV else out.cpu(), ref, _case_id(case))


# ---- every epilogue instantiation on one shape of each family -----------------------------------------------------------------------
def _check_epilogue(op, M, N, K, flags, kernel, wide_disabled=False):
    dev = _where(M, N)
    d = G.epilogue_inputs(op, M, N, K, flags, device=dev)
    A, B = d.pop("A"), d.pop("B")
    d.pop("flags")
    ref, dead = G.gemm_ref64(op, A, B, flags, exact=True, **d)
    out, _, counts = _run(op, A, B, M, N, K, flags, wide_disabled=wide_disabled, **d)
    assert counts == {kernel: 1}, counts
    out = out if dev == DEV else out.cpu()
    if flags & G.TANH:
        # tanhf against float64 tanh of the EXACT pre-activation: the suite's 2e-5 absolute (test_gemm_epilogues); what dropout and the
        # row mask zeroed is exact
        err = float((out.double() - ref).abs().max())
        print(f"{OPN[op]} {M}x{N}x{K} flags {flags}: max |err| {err:.3e}")
        assert not bool(out.isnan().any()) and err <= 2e-5
        base = d["C0"] if flags & G.ACCUM else torch.zeros_like(out)
        assert torch.equal(out[dead], base[dead])
        if not flags & G.ACCUM:
            assert torch.equal(out == 0, ref == 0)
    else:
        _assert_equal(out, ref, f"{OPN[op]} {M}x{N}x{K} flags {flags}")


EPI_PARAMS = [pytest.param(op, shape, wd, kernel, flags, id=f"{OPN[op]}-{shape[0]}x{shape[1]}x{shape[2]}-{kernel[5:-7]}-f{flags}")
              for op in (G.NT, G.NN) for shape, wd, kernel in G.EPILOGUE_SHAPES[op] for flags in G.EPILOGUE_SETS[op]]


@pytest.mark.parametrize("op,shape,wd,kernel,flags", EPI_PARAMS)
def test_every_epilogue_instantiation_is_exact(op, shape, wd, kernel, flags):
    _check_epilogue(op, *shape, flags, kernel, wd)


@pytest.mark.parametrize("op", [G.NT, G.NN], ids=["NT", "NN"])
@pytest.mark.parametrize("shape,wd,kernel", G.LARGE_EPILOGUE_SHAPES, ids=["lds-ntpb8", "wide-ntpb2"])
def test_model_epilogues_are_exact_on_the_large_shapes(op, shape, wd, kernel):
    """B|M|D (fc1's, NT) and R|M|D (the pff backward's, NN) where a workgroup walks several tiles"""
    _check_epilogue(op, *shape, G.LARGE_EPILOGUE_FLAGS[op], kernel, wd)


# ---- TN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["colsum", "plain", "accum"])
@pytest.mark.parametrize("case", G.TN_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}xR{c[0][2]}" + ("-gather" if c[1] else ""))
def test_tn_dense_integers_are_exact(case, mode):
    (M, N, R_), gather, want = case
    path = G.expected_kernel(G.TN, M, N, R_, gather=gather)
    assert path.kernel == want["kernel"]
    g = G.gen(M + 3 * N + 7 * R_)
    A = G.ints(g, (R_, M), 31)
    idx = None
    if gather:
        B = G.ints(g, (500, N), 31)
        idx = torch.randint(0, 500, (R_,), generator=g)
    else:
        B = G.ints(g, (R_, N), 31)
    C0 = col0 = None
    if mode == "accum":
        C0, col0 = G.ints(g, (M, N), 1000), G.ints(g, (M,), 1000)
    ref, refc = G.tn_ref64(A, B, gather=idx, C0=C0, col0=col0, exact=True)
    out, col, counts = _run(G.TN, A, B, M, N, R_, G.ACCUM if mode == "accum" else 0, C0=C0, colsum0=col0, want_colsum=mode != "plain", gather=idx)
    assert counts == {path.kernel: 1, "slab_reduce_kernel": 1}, counts
    _assert_equal(out.cpu(), ref, f"TN {case}")
    if mode != "plain":
        _assert_equal(col.cpu(), refc, f"TN column sums {case}")


# ---- selection inputs: the planes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("op,shape,wd,kernel", G.SELECTION_CASES, ids=[f"{OPN[c[0]]}-{c[1][0]}x{c[1][1]}x{c[1][2]}" for c in G.SELECTION_CASES])
def test_selection_inputs_are_exact(op, shape, wd, kernel, kind):
    M, N, K = shape
    dev = _where(M, N)
    A, B = G.SELECTIONS[kind](op, M, N, K, G.gen(M + N + K + ord(kind), dev))
    ref, _ = G.gemm_ref64(op, A, B, exact=True)
    assert int((ref != 0).sum()) >= ref.numel() // 8
    out, _, counts = _run(op, A, B, M, N, K, wide_disabled=wd)
    assert counts == {kernel: 1}, counts
    _assert_equal(out if dev == DEV else out.cpu(), ref, f"selection ({kind}) {OPN[op]} {shape}")


@pytest.mark.parametrize("shape,kernel", G.SELECTION_TN_CASES, ids=[f"{c[0][0]}x{c[0][1]}xR{c[0][2]}" for c in G.SELECTION_TN_CASES])
def test_tn_selection_inputs_are_exact(shape, kernel):
    M, N, R_ = shape
    A, B = G.selection_tn(M, N, R_, G.gen(M + N + R_))
    ref, _ = G.tn_ref64(A, B, exact=True)
    assert int((ref != 0).sum()) == ref.numel()
    out, _, counts = _run(G.TN, A, B, M, N, R_)
    assert counts == {kernel: 1, "slab_reduce_kernel": 1}, counts
    _assert_equal(out.cpu(), ref, f"TN selection {shape}")


# ---- a graded random case per family ---------------------------------------------------------------------------------------------------
# e(X) = rms(X - R64) / rms(R64) <= GRADE_FACTOR (4) * max(e(R32), 2^-23), R32 = torch's fp32 product on the CPU.  On the CPU the correct
# six-product scheme has e = 0.8e-7 (K = 64) .. 4.9e-7 (K = 2048) against bounds of 5.8e-7 .. 1.16e-6, and any dropped plane has
# e >= 2.4e-6 (tests/test_cpu_gemm_exact.py asserts both sides).  Measured on an MI355X (NT and NN agree to every digit shown; so do the
# staged and the direct f32 kernels, which add the same products in the same order):
#   shape (M, N, K)      bound      gemm_wide_kernel   gemm_lds_kernel        gemm_rm_kernel
#   (300, 64, 64)        5.68e-7    --                 1.43e-7 (BK = 64)      1.43e-7
#   (300, 128, 256)      8.26e-7    2.38e-7            2.84e-7 (BK = 32)      2.84e-7
#   (515, 1536, 192)     9.96e-7    2.04e-7            2.49e-7 (BK = 32)      2.49e-7
#   (130, 128, 2048)     1.02e-6    6.93e-7            8.05e-7 (BK = 32)      8.05e-7
# The six bf16 plane products are, on these inputs, slightly CLOSER to float64 than the f32 MFMA chain; at K = 2048 both use most of the
# bound, as a chain of 2048 f32 additions must (the CPU emulation of the six products gives 4.9e-7 there).
ROUTES = {"default": {}, "nowide": dict(wide_disabled=True), "direct": dict(misalign="A")}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", G.GRADED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_graded_random_case(shape, route):
    M, N, K = shape
    kw = ROUTES[route]
    A, W = G.graded_inputs(M, N, K)
    bound, ref = G.graded_bound(A, W)
    for op, B in ((G.NT, W), (G.NN, W.t().contiguous())):
        path = G.expected_kernel(op, M, N, K, wide_disabled=kw.get("wide_disabled", False), a_aligned="misalign" not in kw)
        out, _, counts = _run(op, A, B, M, N, K, **kw)
        assert counts == {path.kernel: 1}, counts
        e = G.rel_rms(out.cpu(), ref)
        print(f"graded {OPN[op]} {M}x{N}x{K} {route}: {path.kernel} bk={path.bk} e = {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (e, bound)


# ---- K < 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [G.NT, G.NN, G.TN], ids=["NT", "NN", "TN"])
def test_an_empty_contraction_is_refused_before_any_launch(op):
    lib = _lib.load()
    A, B = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    out = torch.full((8, 8), float("nan"), device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for M, N, K, ok in [(8, 8, 0, False), (8, 8, -1, False), (-1, 8, 8, False), (8, -1, 8, False), (0, 8, 8, True), (8, 0, 8, True)]:
        with _lib.launch_log() as log:
            rc = lib.matcha_gemm(op, _lib.ptr(A), _lib.ptr(B), _lib.ptr(out), M, N, K, None, None, None, _lib.ptr(ws), ws.numel(), _stream())
        torch.cuda.synchronize()
        assert (rc == 0) == ok and log.counts == {}, (M, N, K, rc, log.counts)
        assert bool(out.isnan().all())
