"""The denoised contact maps on the MI355X (csrc/denoise.hip + matcha_quantile_uniform, matcha_amd/denoise.py): bit for bit with
the REAL denoise_contact.py (gd_* fixtures) and with tests/denoise_ref.py on synthetic chromosomes, end to end through the
reference-pickled tiny models, deterministic, argument errors refused before any launch, and the CLI."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from matcha_amd import denoise as D
from matcha_amd.predict import pairwise_probabilities
from tests import denoise_ref as R
from tests.helpers import GOLD, rel_err
from tests.test_cpu_denoise import CASES, MATS, fixture, same

pytestmark = pytest.mark.gpu

KERNELS = {"denoise_assemble_kernel", "denoise_row_sums_kernel", "denoise_col_sums_kernel", "denoise_combine_kernel",
           "denoise_finish_kernel", "denoise_pixels_kernel", "quantile_transform_kernel"}
PRE = ["my", "origin_part", "my_proba", "gap1", "gap2"]
TOL = 1e-4                       # the device sweep against the reference's CPU logits (test_predict_consumers.py)
# which reference-pickled tiny model and task mode produced each tiny fixture (tests/golden/make_golden_denoise.py: CASES)
TINY_MODELS = {"tiny_table_md2": ("table", "class"), "tiny_adj_md0": ("adj", "class"), "tiny_table_regress": ("table", "regress")}


def host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def check_equal(got, ref, keys, what):
    for k in keys:
        if ref.get(k) is None:
            continue
        assert same(got[k], ref[k]), f"{what}: {k} differs (max abs {np.max(np.abs(got[k].astype(np.float64) - ref[k])) if got[k].shape == ref[k].shape else got[k].shape})"


def blocks(num, seed):
    intra = R.fixture_intra(num, seed)
    b = synth.bounds(num)
    return [intra[b[c]:b[c + 1], b[c]:b[c + 1]] for c in range(len(num))], intra


def load_tiny(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    return torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False)


@pytest.mark.parametrize("case", CASES)
def test_fixture_bitwise(case):
    """The reference's own probabilities in: every pre-quantile matrix, gap, transformed matrix and pixel equals the fixture."""
    g = fixture(case)
    num, min_dis = [int(v) for v in g["num"]], int(g["min_dis"])
    bl, _ = blocks(num, int(g["seed"]))
    for c, n in enumerate(num):
        got = host(D.denoise_from_proba(torch.from_numpy(g[f"proba_c{c}"]).cuda(), torch.from_numpy(bl[c]).cuda(), n, min_dis,
                                        quantile_proba=True))
        ref = {k: g[f"{k}_c{c}"] for k in MATS if f"{k}_c{c}" in g}
        check_equal(got, ref, list(ref), f"{case} chromosome {c}")


def synthetic(n, min_dis, seed, zero=False):
    rng = np.random.default_rng(seed)
    proba = rng.random(D.pair_count(n, min_dis), dtype=np.float32)
    origin = (rng.gamma(2.0, 1.0, size=(n, n)) / (np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) + 1)).astype(np.float32)
    if zero:
        origin[:] = 0.0
    elif n > 2:
        for k in rng.choice(n, size=max(1, n // 50), replace=False):     # gap rows / columns
            origin[k, :] = 0.0
            origin[:, k] = 0.0
        origin[rng.integers(n), :] = 0.0                                  # a row zeroed only above the diagonal
    return proba, origin


SIZES = [(n, md) for n in (1, 2, 7, 8, 9, 127, 128, 129, 136, 257, 1000, 2491) for md in (0, 2) if n > md]   # n <= md: no pairs


@pytest.mark.parametrize("n,min_dis", SIZES)
def test_synthetic_sizes_bitwise(n, min_dis):
    proba, origin = synthetic(n, min_dis, 1000 * n + min_dis)
    # the origin block as a view into a wider matrix (origin_ld > n)
    wide = torch.zeros(n + 3, n + 5, device="cuda")
    wide[1:n + 1, 2:n + 2] = torch.from_numpy(origin).cuda()
    got = host(D.denoise_from_proba(torch.from_numpy(proba).cuda(), wide[1:, 2:], n, min_dis, quantile_proba=True))
    ref = R.denoise_ref(proba, origin, n, min_dis, quantile_proba=True)
    check_equal(got, ref, MATS, f"n={n} min_dis={min_dis}")


def test_all_zero_origin_bitwise():
    n, min_dis = 300, 2
    proba, origin = synthetic(n, min_dis, 7, zero=True)
    got = host(D.denoise_from_proba(torch.from_numpy(proba).cuda(), torch.from_numpy(origin).cuda(), n, min_dis))
    ref = R.denoise_ref(proba, origin, n, min_dis)
    assert ref["gap1"].all() and ref["gap2"].all()
    check_equal(got, ref, MATS, "all-zero origin")


@pytest.mark.parametrize("n", [8192, 8200])
def test_large_pre_quantile_bitwise(n):
    """n = 8192 (one reduction buffer per row) and 8200 (two: the buffers add in sequence): the pre-quantile matrices and gaps
    bitwise against numpy, the pixels a gather of the device's transformed matrix."""
    min_dis = 2
    proba, origin = synthetic(n, min_dis, n)
    out = D.denoise_from_proba(torch.from_numpy(proba).cuda(), torch.from_numpy(origin).cuda(), n, min_dis)
    pw = torch.from_numpy(R.pairs_ref(0, n, min_dis)).cuda()
    assert torch.equal(out["balanced"], out["my_q"][pw[:, 0], pw[:, 1]])
    got = {k: out[k].cpu().numpy() for k in PRE}
    del out
    torch.cuda.empty_cache()
    pw = R.pairs_ref(0, n, min_dis)
    origin_raw = R.assemble(pw, origin[pw[:, 0], pw[:, 1]], n)
    my_proba = R.coverage(R.assemble(pw, proba, n))
    gap1, gap2 = np.sum(origin_raw, axis=-1) == 0, np.sum(origin_raw, axis=0) == 0
    origin_part = R.coverage(origin_raw)
    del origin_raw
    my = R.coverage(np.maximum(my_proba * origin_part, my_proba))
    for m in (my, my_proba):
        m[gap1, :] = 0.0
        m[:, gap2] = 0.0
    check_equal(got, {"my": my, "origin_part": origin_part, "my_proba": my_proba, "gap1": gap1, "gap2": gap2}, PRE, f"n={n}")


@pytest.mark.parametrize("case", list(TINY_MODELS))
def test_end_to_end_with_reference_models(case):
    g = fixture(case)
    mode, task = TINY_MODELS[case]
    clf = load_tiny(mode)
    num, min_dis = [int(v) for v in g["num"]], int(g["min_dis"])
    cr = np.asarray(synth.chrom_range(num))
    bl, _ = blocks(num, int(g["seed"]))
    for c, n in enumerate(num):
        out = D.denoise_chromosome(clf, cr, c, min_dis, torch.from_numpy(bl[c]).cuda(), task_mode=task)
        proba = out["proba"].cpu().numpy()
        assert rel_err(proba, g[f"proba_c{c}"]) < TOL
        check_equal(host(out), R.denoise_ref(proba, bl[c], n, min_dis), MATS, f"{case} chromosome {c}")


def test_deterministic_and_kernel_set():
    n, min_dis = 1000, 2
    proba, origin = synthetic(n, min_dis, 3)
    p, o = torch.from_numpy(proba).cuda(), torch.from_numpy(origin).cuda()
    with _lib.launch_log() as log:
        a = D.denoise_from_proba(p, o, n, min_dis, quantile_proba=True)
        torch.cuda.synchronize()
    b = D.denoise_from_proba(p, o, n, min_dis, quantile_proba=True)
    for k in MATS:
        assert torch.equal(a[k], b[k]), k
    assert set(log.counts) == KERNELS, log.counts
    assert log.counts["denoise_row_sums_kernel"] == 2 and log.counts["denoise_col_sums_kernel"] == 2
    assert log.counts["quantile_transform_kernel"] == 3 and log.counts["denoise_pixels_kernel"] == 1


def test_no_pairs_launches_nothing():
    for n, min_dis in ((1, 1), (5, 5), (3, 9)):
        with _lib.launch_log() as log:
            out = D.denoise_from_proba(torch.zeros(0, device="cuda"), torch.zeros(n, n, device="cuda"), n, min_dis)
        assert not log.counts and out["balanced"].numel() == 0 and out["my"].numel() == 0


def test_bad_arguments_refused_before_any_launch():
    lib = _lib.load()
    n, min_dis = 64, 2
    K = n - min_dis
    npairs = K * (K + 1) // 2
    proba = torch.zeros(npairs, device="cuda")
    origin = torch.zeros(n, n, device="cuda")
    mats = [torch.zeros(n, n, device="cuda") for _ in range(3)]
    gap = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    wsb = lib.matcha_denoise_workspace_bytes(n)
    assert wsb >= 24 * n and lib.matcha_denoise_workspace_bytes(46341) == 0 and lib.matcha_denoise_workspace_bytes(0) == 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    P = _lib.ptr
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(proba=P(proba), npairs=npairs, n=n, min_dis=min_dis, origin=P(origin), ld=n, my=P(mats[0]), ws=P(ws), wsb=wsb):
        return lib.matcha_denoise_intra(proba, npairs, n, min_dis, origin, ld, my, P(mats[1]), P(mats[2]), P(gap), ws, wsb, st)

    bad = [dict(proba=None), dict(origin=None), dict(my=None), dict(ws=None), dict(n=46341), dict(n=0), dict(npairs=npairs + 1),
           dict(ld=n - 1), dict(wsb=wsb - 1), dict(min_dis=n), dict(min_dis=-1)]
    with _lib.launch_log() as log:
        for kw in bad:
            assert call(**kw) == -22, kw
        assert lib.matcha_denoise_pixels(None, n, min_dis, P(proba), st) == -22
        assert lib.matcha_denoise_pixels(P(mats[0]), n, n, P(proba), st) == -22
    assert not log.counts
    with pytest.raises(ValueError):
        D.denoise_from_proba(proba, torch.zeros(n - 1, n, device="cuda"), n, min_dis)
    assert call() == 0                                                  # the same arguments, corrected, run
    torch.cuda.synchronize()


def _cli_dir(tmp_path, seed, min_dis=2):
    num = R.FIXTURE_LAYOUTS["tiny"]
    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp, exist_ok=True)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    node2bin, names = R.fixture_node2bin(num)
    np.save(os.path.join(temp, "node2bin.npy"), node2bin, allow_pickle=True)
    np.save(os.path.join(temp, "chrom_range.npy"), np.asarray(synth.chrom_range(num)))
    intra = R.fixture_intra(num, seed)
    np.save(os.path.join(temp, "intra_adj.npy"), intra)
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": R.FIXTURE_RES, "chrom_list": names, "min_distance": min_dis}, f)
    return cpath, num, names, intra


@pytest.mark.parametrize("case", ["tiny_table_md2", "tiny_table_regress"])
def test_cli(case, tmp_path):
    g = fixture(case)
    task = TINY_MODELS[case][1]
    cpath, num, names, intra = _cli_dir(tmp_path, int(g["seed"]))
    out_dir = os.path.join(tmp_path, "out")
    D.main(["--config", cpath, "--out-dir", out_dir, "--task-mode", task])
    z = np.load(os.path.join(out_dir, "denoised_pixels.npz"))
    p = "resolutions/%d/" % R.FIXTURE_RES
    for k in ("bins/chrom", "bins/start", "bins/end", "pixels/bin1_id", "pixels/bin2_id"):
        assert np.array_equal(z[p + k], g["ds/" + p + k]), k
    assert [str(s) for s in z[p + "chroms/name"]] == [s.decode() if isinstance(s, bytes) else str(s) for s in g["ds/" + p + "chroms/name"]]
    clf = load_tiny("table")
    cr = np.asarray(synth.chrom_range(num))
    b = synth.bounds(num)
    bal = []
    for c, n in enumerate(num):
        _, proba = pairwise_probabilities(clf, cr, c, 2, task_mode=task)
        proba = proba.cpu().numpy()
        assert rel_err(proba, g[f"proba_c{c}"]) < TOL                  # softplus in regress mode, sigmoid otherwise
        ref = R.denoise_ref(proba, intra[b[c]:b[c + 1], b[c]:b[c + 1]], n, 2)
        bal.append(ref["balanced"])
        assert same(np.load(os.path.join(out_dir, f"{names[c]}_denoise.npy")), ref["my_q"])
        assert same(np.load(os.path.join(out_dir, f"{names[c]}_origin.npy")), ref["origin_q"])
    assert same(z[p + "pixels/balanced"], np.concatenate(bal))


def test_cli_mcool_when_h5py(tmp_path):
    h5py = pytest.importorskip("h5py")
    cpath, num, names, intra = _cli_dir(tmp_path, 81)
    out_dir = os.path.join(tmp_path, "out")
    D.main(["--config", cpath, "--out-dir", out_dir, "--no-matrices"])
    z = np.load(os.path.join(out_dir, "denoised_pixels.npz"))
    with h5py.File(os.path.join(out_dir, "denoised.mcool"), "r") as f:
        for k in z.files:
            if not k.endswith("chroms/name"):
                assert np.array_equal(f[k][()], z[k]), k
    assert not os.path.exists(os.path.join(out_dir, "chr1_denoise.npy"))
