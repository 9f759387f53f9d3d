"""Plain references for matcha_gemm (include/matcha_hip.h) and a Python restatement of its dispatch rule.

Three things live here, shared by tests/test_cpu_gemm_exact.py (no GPU) and tests/test_hip_gemm_exact.py (GPU):

* ``gemm_ref64``: the product in float64 followed by the epilogue in the kernels' fixed order
  (bias -> tanh -> +residual -> dropout -> row mask -> * (1 - (aux * aux_scale)^2) -> accumulate), written with plain torch ops
  so that it runs on the CPU and, for the two large shapes, on the device.  With ``exact=True`` every stage is checked to be
  representable in float32 (``float32(v) == v`` element-wise): a kernel rounds to float32 after every stage, so an input set
  is valid for a bit-for-bit comparison only when no stage rounds.
* input generators whose products and partial sums are exactly representable, in ANY summation order: dense small integers, and
  "selection" operands (one nonzero per row / column) against full-mantissa values, which make every one of the six bf16 plane
  products of the wide kernels individually visible as a bit mismatch.
* ``expected_kernel``: the launch rules of gemm_lds.hip::launch_gemm_rm, gemm_f32.hip::launch_gemm_rm_direct / launch_gemm_tn and
  gemm_wide.hip, restated for the operand layout the entry builds (lda = K, ldb = K or N, ldc = N; for TN lda = M, ldb = N).
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import rng as R

NT, NN, TN = 0, 1, 2
BIAS, TANH, DROPOUT, ROWMASK, RESIDUAL, DTANH, ACCUM = 1, 2, 4, 8, 16, 32, 64
ALL_FLAGS = BIAS | TANH | DROPOUT | ROWMASK | RESIDUAL | DTANH | ACCUM
# the compile-time epilogue instantiations of the two `switch` statements (gemm_lds.hip, gemm_wide.hip); any other set runs the generic -1 one
SPECIALISED = {NT: (0, BIAS, BIAS | TANH, BIAS | TANH | DROPOUT, BIAS | ROWMASK, BIAS | ROWMASK | DROPOUT, BIAS | RESIDUAL),
               NN: (0, DTANH, DTANH | DROPOUT, RESIDUAL | ROWMASK, RESIDUAL | ROWMASK | DROPOUT)}
# every instantiation named in the switches, plus two generic sets per op: ACCUM alone, and all flags
EPILOGUE_SETS = {op: SPECIALISED[op] + (ACCUM, ALL_FLAGS) for op in (NT, NN)}


def epilogue_instance(op, flags):
    return flags if flags in SPECIALISED[op] else -1


def cdiv(a, b):
    return -(-a // b)


# ---- the dispatch rule ----------------------------------------------------------------------------------------------------------
# kernel: the name the launch log reports;  bk: the lds kernel's chunk depth;  vec: the direct kernel's VEC template argument;
# ntpb: tiles per workgroup (lds: column tiles on one resident A tile; wide: consecutive tiles of one pipeline);
# P, rows_per_block: the TN kernels' row partitions;  nwg / launched: the wide kernel's working and launched workgroups
Path = namedtuple("Path", "kernel bk vec ntpb P rows_per_block nwg launched")


def _path(kernel, bk=None, vec=None, ntpb=None, P=None, rows_per_block=None, nwg=None, launched=None):
    return Path(kernel, bk, vec, ntpb, P, rows_per_block, nwg, launched)


def expected_kernel(op, M, N, K, aligned=True, wide_disabled=False, *, a_aligned=None, b_aligned=None, out_aligned=None, gather=False):
    """The kernel matcha_gemm(op, ..., M, N, K) reaches.  ``aligned``: every operand base is 16-byte aligned; a_aligned / b_aligned /
    out_aligned override it for A, B and the epilogue's operands (C, bias, residual, aux).  For TN, K is the row count R."""
    a_al = aligned if a_aligned is None else a_aligned
    b_al = aligned if b_aligned is None else b_aligned
    o_al = aligned if out_aligned is None else out_aligned
    if op == TN:
        R_ = K
        if (not wide_disabled and not gather and M % 128 == 0 and N % 128 == 0 and R_ >= 1 and a_al and b_al):      # gemm_tn_wide_eligible (lda = M, ldb = N)
            tiles = (M // 128) * (N // 128)
            p = max(1, min(cdiv(512, tiles), cdiv(R_, 128)))
            rpb = cdiv(cdiv(R_, p), 32) * 32
            return _path("gemm_tn_wide_kernel", P=max(1, cdiv(R_, rpb)), rows_per_block=rpb)
        tiles = cdiv(M, 64) * cdiv(N, 64)                                                                           # tn_partition
        p = max(1, min(cdiv(1024, tiles), cdiv(R_, 64)))
        rpb = cdiv(cdiv(R_, p), 32) * 32
        return _path("gemm_tn_kernel", P=max(1, cdiv(R_, rpb)), rows_per_block=rpb)
    b_kn = op == NN
    lda, ldb, ldc = K, (N if b_kn else K), N
    vec = lda % 4 == 0 and ldb % 4 == 0 and a_al and b_al and (not b_kn or N % 4 == 0)                               # launch_gemm_rm
    wide = (not wide_disabled and N % 128 == 0 and K % 32 == 0 and K >= 64 and M >= 1 and ldc % 4 == 0 and a_al and b_al and o_al)
    if vec and wide:                                                                                                # launch_wide_one
        nx, ny = N // 128, cdiv(M, 128)
        ntpb = max(1, min(8, (nx * ny) // 2048))
        nwg = cdiv(nx * ny, ntpb)
        return _path("gemm_wide_kernel", ntpb=ntpb, nwg=nwg, launched=cdiv(nwg, 8) * 8)
    if not vec:                                                                                                     # launch_gemm_rm_direct
        v = K % 4 == 0 and lda % 4 == 0 and a_al and (b_kn or (ldb % 4 == 0 and b_al))
        return _path("gemm_rm_kernel", vec=v)
    tiles_n, tiles_m = cdiv(N, 64), cdiv(M, 128)
    ntpb = min(tiles_n, 8) if K <= 64 else 1
    if tiles_m * cdiv(tiles_n, ntpb) < 256:
        ntpb = 1
    return _path("gemm_lds_kernel", bk=64 if K <= 64 else 32, ntpb=ntpb)


# ---- dropout mask: oracle/rng.py's, and the same counter hash in torch integer ops for masks formed on the device -----------------
def _lowbias32_t(x):
    m = 0xFFFFFFFF
    x = x & m
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m          # the int64 product may wrap; its low 32 bits are what is kept
    x = x ^ (x >> 16)
    return x


def dropout_mask_torch(seed, stream, p, n_rows, n_cols, device="cpu"):
    """oracle/rng.py::dropout_mask in torch int64 ops (tests/test_cpu_gemm_exact.py pins the two to each other)."""
    key = int(R.make_key(seed, stream))
    thr = int(R.dropout_threshold(p))
    rows = torch.arange(n_rows, dtype=torch.int64, device=device)[:, None]
    cols = torch.arange(n_cols, dtype=torch.int64, device=device)[None, :]
    r = _lowbias32_t(cols ^ _lowbias32_t(rows ^ key))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.where(r >= thr, torch.tensor(scale, dtype=torch.float32, device=device), torch.tensor(0.0, dtype=torch.float32, device=device))


def assert_f32_exact(v64, what):
    """float32(v) == v element-wise: the assertion that makes an input set valid for a bit-for-bit comparison"""
    bad = v64.float().double() != v64
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values are not representable in float32"


def gemm_ref64(op, A, B, flags=0, *, bias=None, residual=None, aux=None, aux_scale=1.0, row_ids=None, seed=None, stream=None, p=0.0,
               C0=None, exact=False):
    """float64 reference of matcha_gemm.  Returns (C [M,N] float64, dead [M,N] bool): ``dead`` marks the elements dropout or the row mask
    zeroed (their stored value is exactly C0 under EPI_ACCUM, else exactly 0).  For TN use ``tn_ref64``.  Tensors may live on any device."""
    A64, B64 = A.double(), B.double()
    assert op in (NT, NN)
    v = A64 @ (B64.t() if op == NT else B64)
    dead = torch.zeros(v.shape, dtype=torch.bool, device=v.device)

    def stage(name):
        if exact:
            assert_f32_exact(v, name)

    stage("product")
    if flags & BIAS:
        v = v + bias.double()[None, :]
        stage("bias")
    if flags & TANH:
        v = torch.tanh(v)                                    # not exact: TANH cases are compared at a tolerance, see the tests
    if flags & RESIDUAL:
        v = v + residual.double()
        if not flags & TANH:
            stage("residual")
    if flags & DROPOUT:
        mask = dropout_mask_torch(seed, stream, p, v.shape[0], v.shape[1], device=v.device)
        dead |= mask == 0
        v = v * mask.double()
        if not flags & TANH:
            stage("dropout")
    if flags & ROWMASK:
        off = (row_ids == 0)[:, None]
        dead |= off
        v = torch.where(off, torch.zeros_like(v), v)
    if flags & DTANH:
        a = aux.double() * float(np.float32(aux_scale))
        if exact:
            assert_f32_exact(a, "aux * aux_scale")
            assert_f32_exact(1.0 - a * a, "1 - a^2")
        v = v * (1.0 - a * a)
        if not flags & TANH:
            stage("dtanh")
    if flags & ACCUM:
        v = v + C0.double()
        if not flags & TANH:
            stage("accumulate")
    return v, dead


def tn_ref64(A, B, *, gather=None, C0=None, col0=None, exact=False):
    """float64 reference of the TN op: C = A[R,M]^T . B[R,N] (rows of B gathered through ``gather``), column sums of A; C0 / col0 are the
    accumulate bases (EPI_ACCUM accumulates both).  Returns (C, colsum)."""
    Bg = B if gather is None else B[gather]
    c = A.double().t() @ Bg.double()
    cs = A.double().sum(0)
    if exact:
        # every partial sum of a slab or of the fixed-order reduction is a sub-sum of these terms: bounded by the sum of magnitudes
        assert_f32_exact(c, "TN product")
    if C0 is not None:
        c = c + C0.double()
    if col0 is not None:
        cs = cs + col0.double()
    if exact:
        assert_f32_exact(c, "TN accumulate")
    return c, cs


# ---- exact inputs ---------------------------------------------------------------------------------------------------------------
def gen(seed, device="cpu"):
    """a seeded generator; everything below is drawn on the generator's device (the large shapes are drawn on the GPU)"""
    return torch.Generator(device=device).manual_seed(seed)


def ints(g, shape, lim):
    """integers in [-lim, lim] as float32"""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g, device=g.device).float()


def dense_int_bound(K, lim):
    """sum_k |a_k b_k| of dense integers: every partial sum, in any order, is an integer of at most this magnitude (exact below 2^24)"""
    return K * lim * lim


def round_bits(x, bits):
    """float32 values rounded (to nearest, ties away in magnitude) to ``bits`` significant bits"""
    drop = 24 - bits
    u = x.contiguous().view(torch.int32)
    u = (u + (1 << (drop - 1))) & ~((1 << drop) - 1)
    return u.view(torch.float32)


def _pow2(g, n, lo=-6, hi=6):
    e = torch.randint(lo, hi + 1, (n,), generator=g, device=g.device)
    s = torch.randint(0, 2, (n,), generator=g, device=g.device) * 2 - 1
    return torch.ldexp(s.float(), e)


def operand_shapes(op, M, N, K):
    return ((M, K), (N, K)) if op == NT else ((M, K), (K, N))


def selection_b(op, M, N, K, g):
    """(a) B holds one nonzero +-2^e per output column at a random k; A is full-mantissa randn.  C[:, n] = A[:, k_n] * 2^e_n."""
    A = torch.randn(M, K, generator=g, device=g.device)
    kn = torch.randint(0, K, (N,), generator=g, device=g.device)
    val = _pow2(g, N)
    Bnk = torch.zeros(N, K, device=g.device)
    Bnk[torch.arange(N, device=g.device), kn] = val
    return A, (Bnk if op == NT else Bnk.t().contiguous())


def selection_a(op, M, N, K, g):
    """(b) A holds one nonzero +-2^e per row at a random k; B is full-mantissa randn."""
    km = torch.randint(0, K, (M,), generator=g, device=g.device)
    val = _pow2(g, M)
    A = torch.zeros(M, K, device=g.device)
    A[torch.arange(M, device=g.device), km] = val
    Bnk = torch.randn(N, K, generator=g, device=g.device)
    return A, (Bnk if op == NT else Bnk.t().contiguous())


def selection_ab(op, M, N, K, g):
    """(c) one nonzero per row of A and per column of B, drawn from the same few k (row i and column j meet when i = j mod 4), both
    randn rounded to 12 significant bits: a 24-bit product, exact, which needs the h and m planes of both operands."""
    G = min(4, K)
    ks = torch.randperm(K, generator=g, device=g.device)[:G]
    A = torch.zeros(M, K, device=g.device)
    A[torch.arange(M, device=g.device), ks[torch.arange(M, device=g.device) % G]] = round_bits(torch.randn(M, generator=g, device=g.device), 12)
    Bnk = torch.zeros(N, K, device=g.device)
    Bnk[torch.arange(N, device=g.device), ks[torch.arange(N, device=g.device) % G]] = round_bits(torch.randn(N, generator=g, device=g.device), 12)
    return A, (Bnk if op == NT else Bnk.t().contiguous())


def epilogue_inputs(op, M, N, K, flags, device="cpu"):
    """Dense-integer operands and epilogue operands for one flag set: keyword arguments of ``gemm_ref64`` (plus A and B).

    Operands are integers in [-31, 31] ([-15, 15] under EPI_DTANH, whose factors 1 - a^2 in {0, 3/4, 15/16, 1} add four bits), bias /
    residual / C0 integers of magnitude <= 1000, p = 0.5 (keep scale exactly 2), aux in {0, +-0.5, +-1} with aux_scale in {1, 0.5}.
    Under EPI_TANH, B and the bias are scaled by the power of two that brings the exact pre-activation into [-4, 4], and residual / C0
    are integers of magnitude <= 8: the comparison is then at 2e-5 absolute, and half an ulp of float32 must stay below that
    (at magnitude 1000 it is 3e-5; below 32 it is 1e-6)."""
    g = gen(M * 1009 + N * 31 + K * 7 + flags * 131 + op, device)
    sa, sb = operand_shapes(op, M, N, K)
    lim = 15 if flags & DTANH else 31
    small = 8 if flags & TANH else 1000
    d = dict(A=ints(g, sa, lim), B=ints(g, sb, lim), flags=flags)
    if flags & BIAS:
        d["bias"] = ints(g, (N,), small)
    if flags & TANH:
        pre = d["A"].double() @ (d["B"].double().t() if op == NT else d["B"].double())
        if flags & BIAS:
            pre = pre + d["bias"].double()[None, :]
        s = max(0, int(np.ceil(np.log2(float(pre.abs().max()) / 4.0))))
        d["B"] = torch.ldexp(d["B"], torch.tensor(-s, device=device))
        if flags & BIAS:
            d["bias"] = torch.ldexp(d["bias"], torch.tensor(-s, device=device))
    if flags & RESIDUAL:
        d["residual"] = ints(g, (M, N), small)
    if flags & DROPOUT:
        d.update(seed=987654321 + M + flags, stream=R.STREAM_DROP_FC1, p=0.5)
    if flags & ROWMASK:
        d["row_ids"] = torch.randint(0, 3, (M,), generator=g, device=device)
    if flags & DTANH:
        d["aux"] = torch.randint(-2, 3, (M, N), generator=g, device=device).float() * 0.5
        d["aux_scale"] = 0.5 if (M + flags) % 2 else 1.0
    if flags & ACCUM:
        d["C0"] = ints(g, (M, N), small)
    return d


SELECTIONS = {"a": selection_b, "b": selection_a, "c": selection_ab}


def selection_tn(M, N, R_, g):
    """TN: B [R,N] holds one nonzero +-2^e per output column, on N distinct rows spread evenly over [0, R) (so over every row
    partition); all other rows of B are zero.  A [R,M] is full-mantissa randn everywhere.  C[m, n] = A[r_n, m] * 2^e_n."""
    assert R_ >= N
    A = torch.randn(R_, M, generator=g, device=g.device)
    rows = (torch.arange(N, device=g.device) * R_) // N
    assert len(set(rows.tolist())) == N
    B = torch.zeros(R_, N, device=g.device)
    B[rows[torch.randperm(N, generator=g, device=g.device)], torch.arange(N, device=g.device)] = _pow2(g, N)
    return A, B


# ---- the shapes of the exact tests, by the path each must reach -----------------------------------------------------------------
# (id, op, (M, N, K), kwargs of expected_kernel, what misalign to apply, expected fields)
def _c(op, shape, want, wide_disabled=False, misalign=None):
    return dict(op=op, shape=shape, want=want, wide_disabled=wide_disabled, misalign=misalign)


PRODUCT_CASES = [
    # direct kernel (operands that cannot be loaded as aligned 16-byte vectors)
    _c(NT, (131, 70, 66), dict(kernel="gemm_rm_kernel", vec=False)),
    _c(NN, (131, 30, 64), dict(kernel="gemm_rm_kernel", vec=True)),            # N % 4 != 0: VEC on for A, scalar loads for B
    _c(NN, (131, 30, 66), dict(kernel="gemm_rm_kernel", vec=False)),
    _c(NT, (67, 64, 64), dict(kernel="gemm_rm_kernel", vec=False), misalign="A"),
    _c(NT, (67, 64, 64), dict(kernel="gemm_rm_kernel", vec=False), misalign="B"),
    _c(NN, (67, 64, 64), dict(kernel="gemm_rm_kernel", vec=False), misalign="A"),
    _c(NN, (67, 64, 64), dict(kernel="gemm_rm_kernel", vec=True), misalign="B"),
    _c(NT, (1, 1, 5), dict(kernel="gemm_rm_kernel", vec=False)),
    _c(NN, (1, 1, 5), dict(kernel="gemm_rm_kernel", vec=False)),
    # K = 250: the entry passes lda = K, no multiple of 4, so this shape is served by the direct kernel (not by the staged one)
    _c(NT, (257, 24, 250), dict(kernel="gemm_rm_kernel", vec=False)),
    _c(NN, (257, 24, 250), dict(kernel="gemm_rm_kernel", vec=False)),
    # lds kernel, BK = 64 (K <= 64, resident activation tile)
    _c(NT, (37, 16, 16), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1)),
    _c(NN, (37, 16, 16), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1)),
    _c(NT, (129, 72, 40), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1)),      # partial k chunk, partial column tile
    _c(NN, (129, 72, 40), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1)),
    _c(NT, (16300, 520, 40), dict(kernel="gemm_lds_kernel", bk=64, ntpb=8)),   # second column group: one tile of 8 live columns
    _c(NN, (16300, 520, 40), dict(kernel="gemm_lds_kernel", bk=64, ntpb=8)),
    _c(NT, (32700, 128, 64), dict(kernel="gemm_lds_kernel", bk=64, ntpb=2), wide_disabled=True),
    _c(NN, (32700, 128, 64), dict(kernel="gemm_lds_kernel", bk=64, ntpb=2), wide_disabled=True),
    # the wide kernel's fallback when C or the bias is not 16-byte aligned (K = 64: the resident-tile instantiation)
    _c(NT, (129, 128, 64), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1), misalign="C"),
    _c(NT, (129, 128, 64), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1), misalign="bias"),
    _c(NN, (129, 128, 64), dict(kernel="gemm_lds_kernel", bk=64, ntpb=1), misalign="C"),
    # lds kernel, BK = 32 (K > 64)
    _c(NT, (130, 96, 68), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1)),
    _c(NN, (130, 96, 68), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1)),
    _c(NT, (257, 24, 252), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1)),     # (257, 24, 250)'s neighbour with K % 4 == 0: partial last chunk of 28
    _c(NN, (257, 24, 252), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1)),
    _c(NT, (300, 128, 128), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1), wide_disabled=True),
    _c(NN, (300, 128, 128), dict(kernel="gemm_lds_kernel", bk=32, ntpb=1), wide_disabled=True),
    # wide kernel
    _c(NT, (1, 128, 64), dict(kernel="gemm_wide_kernel", ntpb=1)),
    _c(NN, (1, 128, 64), dict(kernel="gemm_wide_kernel", ntpb=1)),
    _c(NT, (257, 256, 96), dict(kernel="gemm_wide_kernel", ntpb=1)),
    _c(NN, (257, 256, 96), dict(kernel="gemm_wide_kernel", ntpb=1)),
    _c(NT, (35073, 1920, 64), dict(kernel="gemm_wide_kernel", ntpb=2, nwg=2063, launched=2064)),
    _c(NN, (35073, 1920, 64), dict(kernel="gemm_wide_kernel", ntpb=2, nwg=2063, launched=2064)),
]

# one shape of each family for the epilogue sets (per op), and the large shapes that additionally run B|M|D (NT) / R|M|D (NN)
EPILOGUE_SHAPES = {
    NT: [((131, 70, 66), False, "gemm_rm_kernel"), ((129, 72, 40), False, "gemm_lds_kernel"), ((130, 96, 68), False, "gemm_lds_kernel"),
         ((257, 256, 96), False, "gemm_wide_kernel")],
    NN: [((131, 30, 66), False, "gemm_rm_kernel"), ((129, 72, 40), False, "gemm_lds_kernel"), ((130, 96, 68), False, "gemm_lds_kernel"),
         ((257, 256, 96), False, "gemm_wide_kernel")],
}
LARGE_EPILOGUE_SHAPES = [((16300, 520, 40), False, "gemm_lds_kernel"), ((35073, 1920, 64), False, "gemm_wide_kernel")]
LARGE_EPILOGUE_FLAGS = {NT: BIAS | ROWMASK | DROPOUT, NN: RESIDUAL | ROWMASK | DROPOUT}

# TN: (M, N, R), gather, expected kernel
TN_CASES = [
    ((30, 50, 1), False, dict(kernel="gemm_tn_kernel", P=1, rows_per_block=32)),
    ((30, 50, 63), False, dict(kernel="gemm_tn_kernel", P=1, rows_per_block=64)),
    ((64, 24, 65), False, dict(kernel="gemm_tn_kernel", P=2, rows_per_block=64)),
    ((70, 130, 1000), False, dict(kernel="gemm_tn_kernel", P=16, rows_per_block=64)),
    ((64, 24, 3000), True, dict(kernel="gemm_tn_kernel", P=47, rows_per_block=64)),
    ((128, 128, 1), False, dict(kernel="gemm_tn_wide_kernel", P=1, rows_per_block=32)),
    ((128, 256, 100), False, dict(kernel="gemm_tn_wide_kernel", P=1, rows_per_block=128)),      # P = 1, partial chunk (100 = 3 x 32 + 4)
    ((256, 128, 229), False, dict(kernel="gemm_tn_wide_kernel", P=2, rows_per_block=128)),
    ((128, 128, 5000), False, dict(kernel="gemm_tn_wide_kernel", P=40, rows_per_block=128)),
]

# selection inputs: one shape per family
SELECTION_CASES = [
    (NT, (131, 70, 66), False, "gemm_rm_kernel"), (NN, (131, 30, 64), False, "gemm_rm_kernel"),
    (NT, (129, 72, 40), False, "gemm_lds_kernel"), (NN, (129, 72, 40), False, "gemm_lds_kernel"),
    (NT, (130, 96, 68), False, "gemm_lds_kernel"), (NN, (130, 96, 68), False, "gemm_lds_kernel"),
    (NT, (257, 256, 96), False, "gemm_wide_kernel"), (NN, (257, 256, 96), False, "gemm_wide_kernel"),
    (NT, (35073, 1920, 64), False, "gemm_wide_kernel"), (NN, (35073, 1920, 64), False, "gemm_wide_kernel"),
]
SELECTION_TN_CASES = [((70, 130, 1000), "gemm_tn_kernel"), ((256, 128, 229), "gemm_tn_wide_kernel"), ((128, 128, 5000), "gemm_tn_wide_kernel")]

# graded random cases (section 4 of the issue): e(X) = rms(X - R64) / rms(R64) <= GRADE_FACTOR * max(e(R32), 2^-23)
GRADED_SHAPES = [(300, 64, 64), (300, 128, 256), (515, 1536, 192), (130, 128, 2048)]
GRADE_FACTOR = 4.0


def rel_rms(x, ref64):
    d = x.double() - ref64
    return float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())


def graded_inputs(M, N, K):
    g = gen(M * 7 + N * 3 + K)
    return torch.randn(M, K, generator=g, device=g.device), torch.randn(N, K, generator=g, device=g.device) * 0.2


def graded_bound(A, W):
    """GRADE_FACTOR * max(e(R32), 2^-23), R32 = torch's fp32 product on the CPU; also returns the float64 reference"""
    ref = A.double() @ W.double().t()
    e32 = rel_rms(A @ W.t(), ref)
    return GRADE_FACTOR * max(e32, 2.0 ** -23), ref
