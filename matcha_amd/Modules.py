"""Host-side mirror of the reference's ``Modules`` interface for the hyperedge-classifier path.

Same class names, constructor arguments, sub-module / parameter names (hence identical ``state_dict()`` keys,
including the odd ``'tied weight_0'`` names) and the same call surface --
``model(x)``, ``model(x, return_recon=True)``, ``model.get_node_embeddings(x)``,
``model.get_embedding(...)``, ``torch.save(model)`` / ``torch.load`` -- as
``/root/reference/Code/Modules.py`` (cited per class below).  What differs is everything underneath: the
sub-modules are parameter containers only, and ``Classifier.forward`` runs the hand-written gfx950 kernels
of ``libmatcha_hip.so`` through the C ABI in ``include/matcha_hip.h``.  There is no PyTorch-op fallback: on a
machine without the library or without a GPU tensor the call raises.

A model pickled by the *reference* (``torch.save(model, "model2load")``, main.py:322/:685) unpickles into these
classes when this module is importable as ``Modules`` (see the top-level ``Modules.py`` shim) and runs on the
HIP path unchanged: the runtime state is rebuilt lazily from the module tree.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import weakref
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib

__all__ = ["Classifier", "MultipleEmbedding", "Wrap_Embedding", "SparseEmbedding", "TiedAutoEncoder",
           "EncoderLayer", "MultiHeadAttention", "ScaledDotProductAttention", "PositionwiseFeedForward",
           "FeedForward", "DataGenerator", "get_non_pad_mask", "get_attn_key_pad_mask"]

_PUBLIC_MODULE = "Modules"   # pickles refer to `Modules.<Class>` exactly like the reference's (main.py:322)

# what Classifier.locus_scores returns: logits [B,1], scores [B,L], order [B,lowest] int64 or None
LocusScores = collections.namedtuple("LocusScores", ["logits", "scores", "order"])


def _default_device() -> torch.device:
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _no_submodule_forward(self, *a, **k):
    raise RuntimeError(
        f"{type(self).__name__} is a parameter container in matcha_amd; the computation runs fused inside "
        "Classifier.forward / get_node_embeddings on the HIP path")


# ----------------------------------------------------------------------------------------------------
# small helpers on the reference's surface
# ----------------------------------------------------------------------------------------------------
def get_non_pad_mask(seq: torch.Tensor) -> torch.Tensor:
    """x != 0 as float [B,L,1] (reference Modules.py:12-14)."""
    if seq.dim() != 2:
        raise AssertionError("expected a [B, L] tensor")
    return (seq != 0).to(torch.float32).unsqueeze(-1)


def get_attn_key_pad_mask(seq_k: torch.Tensor, seq_q: torch.Tensor) -> torch.Tensor:
    """x == 0 expanded to [B, Lq, Lk] (reference Modules.py:17-26).  The reference computes it and then never
    applies it (SURVEY.md headline fact 7); kept for surface compatibility only."""
    return (seq_k == 0).unsqueeze(1).expand(-1, seq_q.size(1), -1)


# ----------------------------------------------------------------------------------------------------
# parameter containers (same registration names and initialisers as the reference)
# ----------------------------------------------------------------------------------------------------
class Wrap_Embedding(nn.Embedding):
    """Trainable bin-embedding table (reference Modules.py:29-34).  Used as ``node_embedding``; its lookup
    (+ zero recon loss) happens inside the fused kernels."""

    def forward(self, *input):
        x = input[0]
        rows = _gather_rows(self.weight, x)
        return rows, torch.zeros(1, dtype=self.weight.dtype, device=self.weight.device)


class SparseEmbedding(nn.Module):
    """Frozen feature matrix holder (reference Modules.py:38-67): ``.embedding`` is a plain tensor attribute
    (not a buffer), so it travels inside the pickle but not in the state_dict."""

    def __init__(self, embedding_weight, sparse=False):
        super().__init__()
        if sparse:
            raise NotImplementedError("sparse (scipy) feature matrices are not supported on the HIP path")
        w = embedding_weight.todense() if hasattr(embedding_weight, "todense") else embedding_weight
        self.sparse = False
        if isinstance(w, torch.Tensor):                      # features built on the device (matcha_amd.features)
            self.embedding = w.detach().contiguous().to(_default_device())
        else:
            self.embedding = torch.from_numpy(np.ascontiguousarray(np.asarray(w))).to(_default_device())

    forward = _no_submodule_forward


class TiedAutoEncoder(nn.Module):
    """Per-chromosome encoder weights (reference Modules.py:70-122): parameters ``'tied weight_%d'``,
    ``'tied bias1'``, ``'tied bias2'`` with the reference's (quirky) registration: for shape_list [n,d,d] the
    surviving biases are bias_list[1] [d] and recon_bias_list[1] [n].  Only the weights are live (use_bias=False
    at Modules.py:163; the decoder output is discarded at :187)."""

    def __init__(self, shape_list, use_bias=True):
        super().__init__()
        dev = _default_device()
        self.use_bias = use_bias
        self.weight_list, self.bias_list, self.recon_bias_list = [], [], []
        for i in range(len(shape_list) - 1):
            self.weight_list.append(nn.Parameter(torch.empty(shape_list[i + 1], shape_list[i], device=dev)))
            self.bias_list.append(nn.Parameter(torch.empty(shape_list[i + 1], device=dev)))
            self.recon_bias_list.append(nn.Parameter(torch.empty(shape_list[i], device=dev)))
        self.recon_bias_list = self.recon_bias_list[::-1]
        for i, w in enumerate(self.weight_list):
            self.register_parameter("tied weight_%d" % i, w)
            self.register_parameter("tied bias1", self.bias_list[i])
            self.register_parameter("tied bias2", self.recon_bias_list[i])
        self.reset_parameters()

    def reset_parameters(self):
        for w in self.weight_list:
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        for w, b in zip(self.weight_list, self.bias_list):
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(w)
            nn.init.uniform_(b, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
        for w, b in zip(self.weight_list[::-1], self.recon_bias_list):
            _, fan_out = nn.init._calculate_fan_in_and_fan_out(w)
            nn.init.uniform_(b, -1 / math.sqrt(fan_out), 1 / math.sqrt(fan_out))

    forward = _no_submodule_forward


class FeedForward(nn.Module):
    """Linear stack ``FF_Linear%d`` (reference Modules.py:385-414)."""

    def __init__(self, dims, dropout=None, reshape=False, use_bias=True):
        super().__init__()
        self.w_stack = []
        for i in range(len(dims) - 1):
            self.w_stack.append(nn.Linear(dims[i], dims[i + 1], use_bias))
            self.add_module("FF_Linear%d" % i, self.w_stack[-1])
        self.dropout = nn.Dropout(dropout) if dropout is not None else None
        self.reshape = reshape

    forward = _no_submodule_forward


class PositionwiseFeedForward(nn.Module):
    """Conv1d(k=1) stack ``PWF_Conv%d`` + LayerNorm (reference Modules.py:327-376)."""

    def __init__(self, dims, dropout=None, reshape=False, use_bias=True, residual=False, layer_norm=False):
        super().__init__()
        self.w_stack = []
        self.dims = dims
        for i in range(len(dims) - 1):
            self.w_stack.append(nn.Conv1d(dims[i], dims[i + 1], 1, bias=use_bias))
            self.add_module("PWF_Conv%d" % i, self.w_stack[-1])
        self.reshape = reshape
        self.layer_norm = nn.LayerNorm(dims[-1])
        self.dropout = nn.Dropout(dropout) if dropout is not None else None
        self.residual = residual
        self.layer_norm_flag = layer_norm

    forward = _no_submodule_forward


class ScaledDotProductAttention(nn.Module):
    """Holds the temperature only (reference Modules.py:417-460)."""

    def __init__(self, temperature):
        super().__init__()
        self.temperature = temperature

    forward = _no_submodule_forward


class MultiHeadAttention(nn.Module):
    """w_qs / w_ks / w_vs / fc1 / fc2 / layer_norm1-3 (reference Modules.py:463-575)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout, diag_mask, input_dim):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(input_dim, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(input_dim, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(input_dim, n_head * d_v, bias=False)
        nn.init.normal_(self.w_qs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_ks.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_vs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_v)))
        self.attention = ScaledDotProductAttention(temperature=np.power(d_k, 0.5))
        self.fc1 = nn.Linear(n_head * d_v, d_model)
        self.fc2 = nn.Linear(n_head * d_v, d_model)      # dead in the reference's forward (Modules.py:573, :617)
        self.layer_norm1 = nn.LayerNorm(input_dim)
        self.layer_norm2 = nn.LayerNorm(input_dim)
        self.layer_norm3 = nn.LayerNorm(input_dim)
        self.dropout = nn.Dropout(dropout) if dropout is not None else dropout
        self.diag_mask_flag = diag_mask
        self.diag_mask = None

    forward = _no_submodule_forward


class EncoderLayer(nn.Module):
    """mul_head_attn + pff_n1 (+ dead pff_n2) (reference Modules.py:578-617)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout_mul, dropout_pff, diag_mask, bottle_neck):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.mul_head_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout_mul, diag_mask=diag_mask,
                                                input_dim=bottle_neck)
        self.pff_n1 = PositionwiseFeedForward([d_model, d_model, d_model], dropout=dropout_pff, residual=True, layer_norm=True)
        self.pff_n2 = PositionwiseFeedForward([bottle_neck, d_model, d_model], dropout=dropout_pff, residual=False, layer_norm=True)

    forward = _no_submodule_forward


class MultipleEmbedding(nn.Module):
    """adj-mode front end (reference Modules.py:125-201): per-chromosome feature matrices + 2-layer encoders
    ``Embedding_Linear{i}`` and reconstruction heads ``Embedding_recon{i}``; ``inter_initial`` rows are
    z-scored over their positive entries at construction (Modules.py:146-152), in place like the reference."""

    def __init__(self, embedding_weights, dim, sparse=True, num_list=None, chrom_range=None, inter_initial=None):
        super().__init__()
        dev = _default_device()
        self.chrom_range = chrom_range
        self.num_list = torch.tensor([0] + [int(v) for v in list(num_list)]).to(dev)
        self.dim = dim
        self.embeddings = [SparseEmbedding(w, sparse) for w in embedding_weights]
        if isinstance(inter_initial, torch.Tensor):          # raw inter matrix already on the device: z-score there, in place
            from . import features
            self.inter_initial = SparseEmbedding(features.zscore_rows_(inter_initial), sparse)
        elif inter_initial is not None:                      # numpy input: the reference's own host statements
            for i in range(len(inter_initial)):
                row = inter_initial[i, :]
                pos = row > 0
                v = row[pos]
                if v.size:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        inter_initial[i, pos] = ((v - v.mean()) / v.std()).astype("float32")
            inter_initial[np.isnan(inter_initial)] = 0.0
            self.inter_initial = SparseEmbedding(inter_initial, sparse)
        else:
            self.inter_initial = SparseEmbedding(embedding_weights[-1], sparse)
        self.input_size = [int(e.embedding.shape[-1]) for e in self.embeddings]
        self.wstack = [TiedAutoEncoder([self.input_size[i], self.dim, self.dim], use_bias=False).to(dev)
                       for i in range(len(self.embeddings))]
        self.next_w = FeedForward([self.dim, self.dim]).to(dev)     # dead in the reference's forward
        self.recon = [FeedForward([self.dim, int(v[1] - v[0])]).to(dev) for v in self.chrom_range]
        for i, w in enumerate(self.wstack):
            self.add_module("Embedding_Linear%d" % i, w)
            self.add_module("Embedding_recon%d" % i, self.recon[i])
        self.dropout = nn.Dropout(0.2)

    forward = _no_submodule_forward


# ----------------------------------------------------------------------------------------------------
# runtime: flat parameter storage + C-ABI descriptors, rebuilt lazily from the module tree
# ----------------------------------------------------------------------------------------------------
def _gather_rows(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    if not table.is_cuda:
        raise _lib.MatchaHipError("matcha_amd runs on the GPU only: move the model with .to('cuda') (no CPU fallback)")
    lib = _lib.load()
    ids = ids.to(device=table.device, dtype=torch.long).contiguous()
    d = table.shape[1]
    out = torch.empty(ids.numel(), d, dtype=torch.float32, device=table.device)
    shp = _lib.Shape(d, 1, table.shape[0] - 1, 0, 0, 0)
    ten = _lib.Tensors()
    ten.table = table.data_ptr()
    fro = _lib.Frozen()
    status = torch.zeros(4, dtype=torch.int32, device=table.device)
    _lib.check(lib.matcha_node_embeddings(C.byref(shp), C.byref(ten), C.byref(fro), _lib.ptr(ids), ids.numel(), _lib.ptr(out),
                                          None, 0, _lib.ptr(status), C.c_void_p(torch.cuda.current_stream(table.device).cuda_stream)),
               "matcha_node_embeddings")
    _lib.raise_on_status(status.tolist(), "Wrap_Embedding.forward")
    return out.view(*ids.shape, d)


ATTR_COMPUTE = True     # tests flip these two to reach the other attribute-row paths with the same model
ATTR_PAD = True


def _attr_structure(table: torch.Tensor):
    """(bounds, scale) when ``table`` [N+1, A] is what get_attributes (main.py:497-512) builds -- row 0 zeros; row id: a one-hot
    chromosome column c(id) in the first A-1 columns, the chromosomes' ids forming consecutive ranges in column order, and a last
    column float32(id - 1 - first id of the chromosome) / float32(scale) -- checked for EVERY row, bit for bit; None otherwise.
    bounds = [0, n_0, n_0 + n_1, ..., N] (A entries), scale = num[0]."""
    if table.dim() != 2 or table.shape[1] < 2 or table.shape[1] > 64 or table.shape[0] < 2:
        return None
    A = table.shape[1]
    if bool((table[0] != 0).any()):
        return None
    body = table[1:]
    hot = body[:, :A - 1]
    if not bool(((hot == 0) | (hot == 1)).all()) or not bool((hot.sum(1) == 1).all()):
        return None
    col = hot.argmax(1)
    step = col[1:] - col[:-1]
    if bool((step < 0).any()):
        return None
    counts = torch.bincount(col, minlength=A - 1).cpu().tolist()
    bounds = [0]
    for c in counts:
        bounds.append(bounds[-1] + int(c))
    lo = torch.tensor(bounds[:-1], dtype=torch.int64, device=table.device)[col]
    j = torch.arange(body.shape[0], device=table.device, dtype=torch.int64) - lo          # bin index inside its chromosome
    coord = body[:, A - 1]
    nz = torch.nonzero(j > 0)
    if nz.numel() == 0:
        scale = 1.0
    else:
        i0 = int(nz[0])
        c0 = float(coord[i0])
        if c0 <= 0:
            return None
        scale = float(round(float(j[i0]) / c0))
        if scale < 1:
            return None
    want = j.to(torch.float32) / torch.tensor(scale, dtype=torch.float32, device=table.device)   # IEEE float32 division, like numpy's
    if not bool((want == coord).all()):
        return None
    return bounds, scale


class _Runtime:
    """Flat storage for the LIVE parameters (one buffer -> one AdamW launch, one all-reduce bucket) plus the
    ctypes descriptors handed to the C ABI, and derived copies of the FROZEN inputs: the attribute table
    (padded to 32 floats, with the attr_mode / attr_bounds / attr_scale decision taken from it) and, on the adj front
    end, the re-packed feature blocks; inter_initial is a copy or, when it already is float32 on the device, an alias.

    What keeps it valid (``still_packed``; tests/test_hip_state.py part A):
    * live parameters are views into ``flat``: in-place writes (``load_state_dict``, optimizers, ``copy_``) need no
      rebuild -- the kernels read the new values; a parameter whose storage MOVED (``p.data = ...``, a device change,
      unpickling, ``deepcopy``) makes the runtime stale;
    * frozen inputs are tracked by (data_ptr, _version) of the tensor the module tree holds at the time of the call, looked up from
      the model itself (``model.attribute_dict_embedding.weight``, ``model.node_embedding.embeddings[i].embedding``,
      ``.inter_initial.embedding``): ``load_state_dict``, an in-place ``copy_``, the assignment of a new tensor / Parameter and the
      replacement of one of these sub-modules as a whole are all seen.  A rewrite
      of the attribute table with the SAME bytes (train() reloads its checkpoint at the end of every phase) is accepted
      after one device compare per version bump; any other change makes the runtime stale.
    A stale runtime is rebuilt by ``Classifier._runtime()`` on the model's next call, with every derived quantity taken
    again from the new tensors; a Trainer holds on to the runtime it was built with and raises instead.
    NOT detectable: an in-place edit through ``.data`` (``w.data.add_(1)``) bumps no version counter.  For a live parameter
    that is harmless (the kernels read the storage itself); for a frozen input the derived copies go stale silently, so
    change frozen inputs through one of the tracked paths only.  There is deliberately no per-call device compare.  Live parameters
    are tracked by OBJECT: assigning a new ``nn.Parameter`` (or a new sub-module) in place of a live one is not seen either; write
    into the existing parameter instead.
    Cost: the table front end compares one pair of integers per call.  The adj front end builds a tuple of n_chrom + 1 such pairs per
    model call / eager Trainer step (host Python, no device work); its effect on eager adj steps has not been measured -- bench.py times
    the table front end, and captured replays do not pass through here."""

    def __init__(self, model: "Classifier"):
        self.lib = _lib.load()
        dev = model.layer_norm1.weight.device
        if dev.type != "cuda":
            raise _lib.MatchaHipError("matcha_amd runs on the GPU only: move the model with .to('cuda') (no CPU fallback)")
        self.device = dev
        ne = model.node_embedding
        self.mode = 1 if isinstance(ne, MultipleEmbedding) or hasattr(ne, "wstack") else 0
        enc, mha, pff = model.encode1, model.encode1.mul_head_attn, model.encode1.pff_n1
        d = int(model.layer_norm1.weight.shape[0])
        self.d = d
        attr_mod = model.attribute_dict_embedding
        self.n_attr = int(attr_mod.weight.shape[1])
        # (field, [params...], group)  -- group indexes the `touched` flags of matcha_backward
        entries = []
        if self.mode == 0:
            self.n_nodes = int(ne.weight.shape[0]) - 1
            self.n_chrom = 0
            self.max_bins = 0
            entries.append(("table", [ne.weight], 1))
        else:
            bounds = [int(v) for v in ne.num_list.tolist()]
            self.bounds_list = bounds
            self.n_chrom = len(bounds) - 1
            self.n_nodes = bounds[-1]
            self.max_bins = max(bounds[i + 1] - bounds[i] for i in range(self.n_chrom))
            Cn = self.n_chrom
            entries.append(("adj_w0", [getattr(ne.wstack[i], "tied weight_0") for i in range(Cn)], [2 + i for i in range(Cn)]))
            entries.append(("adj_w1", [getattr(ne.wstack[i], "tied weight_1") for i in range(Cn)], [2 + i for i in range(Cn)]))
            entries.append(("recon_w", [ne.recon[i].FF_Linear0.weight for i in range(Cn)], [2 + Cn + i for i in range(Cn)]))
            entries.append(("recon_b", [ne.recon[i].FF_Linear0.bias for i in range(Cn)], [2 + Cn + i for i in range(Cn)]))
        ff = model.next_w.FF_Linear0
        entries += [
            ("attr_w", [model.attribute_nn.weight], 0), ("attr_b", [model.attribute_nn.bias], 0),
            ("next_w", [ff.weight], 0), ("next_b", [ff.bias], 0),
            ("ln_q_g", [mha.layer_norm1.weight], 0), ("ln_q_b", [mha.layer_norm1.bias], 0),
            ("ln_k_g", [mha.layer_norm2.weight], 0), ("ln_k_b", [mha.layer_norm2.bias], 0),
            ("ln_v_g", [mha.layer_norm3.weight], 0), ("ln_v_b", [mha.layer_norm3.bias], 0),
            ("w_q", [mha.w_qs.weight], 0), ("w_k", [mha.w_ks.weight], 0), ("w_v", [mha.w_vs.weight], 0),
            ("fc1_w", [mha.fc1.weight], 0), ("fc1_b", [mha.fc1.bias], 0),
            ("pff0_w", [pff.PWF_Conv0.weight], 0), ("pff0_b", [pff.PWF_Conv0.bias], 0),
            ("pff1_w", [pff.PWF_Conv1.weight], 0), ("pff1_b", [pff.PWF_Conv1.bias], 0),
            ("pff_ln_g", [pff.layer_norm.weight], 0), ("pff_ln_b", [pff.layer_norm.bias], 0),
            ("ln1_g", [model.layer_norm1.weight], 0), ("ln1_b", [model.layer_norm1.bias], 0),
            ("ln2_g", [model.layer_norm2.weight], 0), ("ln2_b", [model.layer_norm2.bias], 0),
            ("cls_w", [model.pff_classifier.PWF_Conv0.weight], 0), ("cls_b", [model.pff_classifier.PWF_Conv0.bias], 0),
        ]
        # flat layout: every ABI field starts on a 16-byte boundary; tensors of one field are back to back
        self.live: List[nn.Parameter] = []
        self.field_off: Dict[str, int] = {}
        seg_off, seg_group = [], []
        off = 0
        for field, plist, group in entries:
            off = (off + 3) // 4 * 4
            self.field_off[field] = off
            for j, p in enumerate(plist):
                seg_off.append(off)
                seg_group.append(group[j] if isinstance(group, list) else group)
                self.live.append(p)
                off += p.numel()
        self.n_flat = (off + 3) // 4 * 4
        seg_off.append(self.n_flat)
        self.seg_off_list, self.seg_group_list = seg_off, seg_group
        self.flat = torch.zeros(self.n_flat, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.live, seg_off[:-1]):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.detach().to(device=dev, dtype=torch.float32))
                p.data = view
        self.expected_ptrs = [p.data_ptr() for p in self.live]
        self.seg_off = torch.tensor(seg_off, dtype=torch.int64, device=dev)
        self.seg_group = torch.tensor(seg_group, dtype=torch.int32, device=dev)
        self.n_touched = 2 + 2 * self.n_chrom
        # frozen inputs.  The kernels work on PRIVATE copies of them (the table padded to 32 floats, the feature blocks re-packed) and on
        # structure decided from the table once, so the runtime remembers which tensor state -- (data_ptr, _version) of what the module
        # tree holds NOW, read from the MODEL at call time (a weak reference: the model owns the runtime), not through a tensor or a
        # sub-module captured here -- those copies were taken from (still_packed)
        self._model = weakref.ref(model)
        self.attr_table = attr_mod.weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        if self.attr_table.data_ptr() == attr_mod.weight.data_ptr():
            self.attr_table = self.attr_table.clone()         # a float32 table already on the device: .to() / .contiguous() return the weight itself
        self._attr_ref = self.attr_table                      # the unpadded private copy the structure decision is taken from: a snapshot, never the live weight
        self._attr_src_state = self._tensor_state(attr_mod.weight)
        self._keep = [self.attr_table]
        self.frozen = _lib.Frozen()
        self.frozen.attr_table = self.attr_table.data_ptr()
        # attribute rows: when the table has the structure main.py:497-512 builds (one-hot chromosome || bin index / num[0]) the kernels
        # rebuild a token's row from its node id instead of gathering it (attr_mode 1: one random row per token); any other
        # table is read as rows padded to 32 floats = one 128-byte fetch unit (a 96-byte row straddles two units three times out of four)
        st = _attr_structure(self.attr_table) if ATTR_COMPUTE else None
        self.attr_mode = 0
        if st is not None:
            bounds, scale = st
            self.attr_bounds = torch.tensor(bounds, dtype=torch.int32, device=dev)
            self.frozen.attr_mode, self.frozen.attr_scale = 1, float(scale)
            self.frozen.attr_bounds = self.attr_bounds.data_ptr()
            self.attr_mode = 1
            self._keep.append(self.attr_bounds)
        # (the table stays available under attr_mode 1: the fused embed_dim-64 forward rebuilds a row from its node id and never reads
        # it, while front_bwd_kernel and the layer-by-layer path -- embed_fwd_kernel, the attribute_nn weight-gradient product -- still
        # gather its rows.  Bounds, scale and table are therefore always derived from ONE snapshot, here)
        if self.n_attr < 32 and ATTR_PAD:
            self.attr_table = torch.nn.functional.pad(self.attr_table, (0, 32 - self.n_attr)).contiguous()
            self._keep[0] = self.attr_table
            self.frozen.attr_table, self.frozen.attr_ld = self.attr_table.data_ptr(), 32
        if self.mode == 1:
            feats = [e.embedding.detach().to(device=dev, dtype=torch.float32).contiguous() for e in ne.embeddings]
            offs = np.zeros(self.n_chrom + 1, dtype=np.int64)
            # every feature row padded with zeros to a multiple of 64 floats (matcha_frozen.feat_row_pad): the gather-GEMMs read
            # aligned 16-byte pieces and a 64-column K chunk never needs a tail mask
            pad = _lib.FEAT_ROW_PAD
            for i, f in enumerate(feats):
                n_i = self.bounds_list[i + 1] - self.bounds_list[i]
                if tuple(f.shape) != (n_i, n_i):
                    raise ValueError("adj mode expects square [n_i, n_i] feature matrices (main.py:571-577)")
                feats[i] = torch.nn.functional.pad(f, (0, (n_i + pad - 1) // pad * pad - n_i))
                offs[i + 1] = offs[i] + feats[i].numel()
            self.feat_pack = torch.cat([f.reshape(-1) for f in feats])
            self.frozen.feat_row_pad = pad
            self.feat_off_host = offs
            self.inter = ne.inter_initial.embedding.detach().to(device=dev, dtype=torch.float32).contiguous()
            self.bounds_dev = torch.tensor(self.bounds_list, dtype=torch.int32, device=dev)
            self.bounds_host = np.asarray(self.bounds_list, dtype=np.int32)
            self.frozen.bounds = self.bounds_dev.data_ptr()
            self.frozen.feats = self.feat_pack.data_ptr()
            self.feat_off_dev = torch.from_numpy(offs).to(dev)
            self.frozen.feat_off = self.feat_off_dev.data_ptr()
            self.frozen.inter = self.inter.data_ptr()
            self.frozen.bounds_host = self.bounds_host.ctypes.data
            self._keep += [self.feat_pack, self.inter, self.bounds_dev, self.feat_off_dev]
            # the reference reads embeddings[i].embedding and inter_initial.embedding on every forward; feat_pack is a re-packed copy
            # and `inter` a copy or an alias: remember the state they were taken from
            self._adj_src_state = self._adj_state(ne)
        self.shape = _lib.Shape(d, self.n_attr, self.n_nodes, self.n_chrom, self.mode, self.max_bins)
        self.params = self.tensors_for(self.flat)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed_counter = 0
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)       # device status word of the id-indexed kernels

    def check_status(self, what: str):
        """Read the device status word (ONE small device-to-host copy, i.e. a synchronisation), clear it and raise what the
        reference raises for a node id outside the tables (IndexError from nn.Embedding, Modules.py:34/:67)."""
        st = self.status.tolist()
        if st[0]:
            self.status.zero_()
            _lib.raise_on_status(st, what)

    def field_off_after(self, field: str) -> int:
        """Element offset of the first ABI field behind ``field`` in the flat buffer (fields start on 16-byte boundaries)."""
        offs = sorted(self.field_off.values())
        i = offs.index(self.field_off[field])
        return offs[i + 1] if i + 1 < len(offs) else self.n_flat

    def tensors_for(self, flat: torch.Tensor) -> "_lib.Tensors":
        t = _lib.Tensors()
        base = flat.data_ptr()
        for field, off in self.field_off.items():
            setattr(t, field, base + 4 * off)
        return t

    @staticmethod
    def _tensor_state(t: torch.Tensor):
        return (t.data_ptr(), t._version)

    def _adj_state(self, ne):
        if not hasattr(ne, "embeddings"):
            return None             # the front end was replaced by another kind: stale
        return tuple(self._tensor_state(e.embedding) for e in ne.embeddings) + (self._tensor_state(ne.inter_initial.embedding),)

    def still_packed(self) -> bool:
        """True while the runtime's view of the model is valid: the live parameters still sit where the kernels were told, and the
        frozen inputs the runtime keeps derived copies of -- the attribute table (padded copy, attr_mode / bounds / scale), on the adj
        front end the feature blocks (feat_pack) and inter_initial -- are the tensors, in the state, the copies were taken from.
        Otherwise the owner rebuilds the runtime (Classifier._runtime) or refuses to go on (Trainer).  Two tuples of integers are
        compared per call: no device work and no synchronisation on a call where nothing changed."""
        model = self._model()
        if model is None:
            return False
        w = model.attribute_dict_embedding.weight
        state = self._tensor_state(w)
        if state != self._attr_src_state:
            # a version bump alone is not a change: train() ends every phase with load_state_dict(model_link), which copy_()s the same bytes
            # into the frozen table.  Compare ONCE per bump (one synchronising device compare, against the private snapshot)
            # and accept an identical table.
            src = w.detach()
            if tuple(src.shape) != tuple(self._attr_ref.shape) or not torch.equal(src.to(device=self.device, dtype=torch.float32), self._attr_ref):
                return False
            self._attr_src_state = state
        if self.mode == 1 and self._adj_state(model.node_embedding) != self._adj_src_state:
            return False            # (nothing rewrites these with the same bytes -- they are not in the state dict --, so any change rebuilds)
        return all(p.data_ptr() == e for p, e in zip(self.live, self.expected_ptrs))

    def workspace(self, B: int, L: int, forward_only: bool = False, long_rows: bool = False, long_train: bool = False) -> torch.Tensor:
        query = self.lib.matcha_workspace_bytes_forward if forward_only else self.lib.matcha_workspace_bytes
        if long_rows:      # rows of 9 .. MAX_LONG_L columns: the long forward has a layout of its own ...
            query = self.lib.matcha_workspace_bytes_long
        if long_train:     # ... and so has the pair matcha_forward_long_train / matcha_backward_long, which keeps the activations
            query = self.lib.matcha_workspace_bytes_long_train
        n = query(C.byref(self.shape), B, L)
        if n == 0:
            raise _lib.MatchaHipError(self.lib.matcha_last_error().decode())
        ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        # development: a read of workspace bytes nobody wrote shows up as NaN / garbage -- the Trainer's workspaces and the ones model(x) takes
        # per call (the autograd path's forward and backward are two calls on one of these)
        if os.environ.get("MATCHA_POISON_WS"):
            ws.fill_(0xFF if os.environ["MATCHA_POISON_WS"] == "nan" else 0x5B)
        return ws

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


def _grad_outputs(rt: "_Runtime", gflat: torch.Tensor, touched: torch.Tensor):
    """The per-parameter gradient views of a backward's flat buffer.  adj front end: the reference leaves .grad None for the encoders /
    recon heads of chromosomes that did not occur in the batch, and torch.optim.AdamW skips such tensors (no weight decay, no moment
    decay): reproducing that through autograd needs the flags on the host, i.e. one synchronisation per backward of THIS path
    (loss.backward() with torch optimisers).  The training path proper (engine.Trainer) keeps the flags on the device and never
    synchronises."""
    tl = touched.tolist() if rt.mode == 1 else None
    outs = []
    for p, o, g in zip(rt.live, rt.seg_off_list[:-1], rt.seg_group_list):
        if tl is not None and g >= 2 and tl[g] == 0:
            outs.append(None)
        else:
            outs.append(gflat[o:o + p.numel()].view(p.shape))
    return outs


class _ClassifierFn(torch.autograd.Function):
    """Autograd glue around matcha_forward / matcha_backward (one node for the whole model)."""

    @staticmethod
    def forward(ctx, x, rt: _Runtime, opts: "_lib.StepOpts", seed_t, *live):
        B, L = x.shape
        ws = rt.workspace(B, L, forward_only=bool(opts.forward_only))      # inference: ~1 KB per token instead of ~20 KB
        logits = torch.empty(B, dtype=torch.float32, device=rt.device)
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        opts.status = rt.status.data_ptr()
        _lib.check(rt.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                         None, None, _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream()),
                   "matcha_forward")
        ctx.rt, ctx.opts, ctx.ws, ctx.x, ctx.seed_t = rt, opts, ws, x, seed_t
        return logits.view(B, 1), losses[1:2]

    @staticmethod
    def backward(ctx, dlogits, drecon):
        rt, opts, x = ctx.rt, ctx.opts, ctx.x
        B, L = x.shape
        if ctx.ws is None:      # matcha_backward overwrites the saved activations with their gradients (include/matcha_hip.h)
            raise RuntimeError("matcha_amd: second backward through the same forward (retain_graph=True is not supported: "
                               "the backward pass consumes the forward's workspace, as torch frees its saved tensors)")
        gflat = torch.zeros(rt.n_flat, dtype=torch.float32, device=rt.device)
        grads = rt.tensors_for(gflat)
        touched = torch.zeros(rt.n_touched, dtype=torch.int32, device=rt.device)
        dl = dlogits.reshape(-1).to(torch.float32).contiguous()
        dr = drecon.reshape(-1).to(torch.float32).contiguous() if drecon is not None else None
        _lib.check(rt.lib.matcha_backward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                          None, None, _lib.ptr(dl), _lib.ptr(dr), C.byref(grads), _lib.ptr(touched), _lib.ptr(ctx.ws),
                                          ctx.ws.numel(), rt.stream()), "matcha_backward")
        ctx.ws = None
        return (None, None, None, None, *_grad_outputs(rt, gflat, touched))


class _ClassifierLongFn(torch.autograd.Function):
    """Autograd glue around matcha_forward_long_train / matcha_backward_long: rows of 9 .. MAX_LONG_L columns, the surface of _ClassifierFn."""

    @staticmethod
    def forward(ctx, x, rt: _Runtime, opts: "_lib.StepOpts", seed_t, *live):
        B, L = x.shape
        ws = rt.workspace(B, L, long_train=True)
        logits = torch.empty(B, dtype=torch.float32, device=rt.device)
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        opts.status = rt.status.data_ptr()
        _lib.check(rt.lib.matcha_forward_long_train(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                                    _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream()),
                   "matcha_forward_long_train")
        ctx.rt, ctx.opts, ctx.ws, ctx.x, ctx.seed_t = rt, opts, ws, x, seed_t
        return logits.view(B, 1), losses[1:2]

    @staticmethod
    def backward(ctx, dlogits, drecon):
        rt, opts, x = ctx.rt, ctx.opts, ctx.x
        B, L = x.shape
        if ctx.ws is None:
            raise RuntimeError("matcha_amd: second backward through the same forward (retain_graph=True is not supported: "
                               "the backward pass consumes the forward's workspace, as torch frees its saved tensors)")
        gflat = torch.zeros(rt.n_flat, dtype=torch.float32, device=rt.device)
        grads = rt.tensors_for(gflat)
        touched = torch.zeros(rt.n_touched, dtype=torch.int32, device=rt.device)
        dl = dlogits.reshape(-1).to(torch.float32).contiguous()
        dr = drecon.reshape(-1).to(torch.float32).contiguous() if drecon is not None else None
        _lib.check(rt.lib.matcha_backward_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                               _lib.ptr(dl), _lib.ptr(dr), C.byref(grads), _lib.ptr(touched), _lib.ptr(ctx.ws),
                                               ctx.ws.numel(), rt.stream()), "matcha_backward_long")
        ctx.ws = None
        return (None, None, None, None, *_grad_outputs(rt, gflat, touched))


class Classifier(nn.Module):
    """Hyper-SAGNN hyperedge classifier (reference Modules.py:204-318): same constructor, parameters and call
    surface; forward = fused gfx950 kernels.  ``model(x)`` returns LOGITS [B,1] (callers apply sigmoid, as in
    main.py:58 / predict_multiway.py:113).

    A call's result depends on the module tree as it is AT the call: train() / eval(), every ``Dropout.p``, the live
    parameters and the frozen inputs (attribute table, adj feature blocks, inter_initial) are read per call, and a
    model changed after its first forward through ``load_state_dict``, ``copy_``, tensor assignment, ``.to()``,
    ``deepcopy`` or pickling behaves like a freshly built one (``_Runtime`` says how, and what is not detectable)."""

    def __init__(self, n_head, d_model, d_k, d_v, node_embedding, diag_mask, bottle_neck, attribute_dict=None, **args):
        super().__init__()
        if n_head != _lib.N_HEAD or not (d_model == d_k == d_v == bottle_neck) or not diag_mask:
            raise NotImplementedError("the HIP path implements the configuration main.py:615-623 builds: "
                                      "n_head=8, d_model=d_k=d_v=bottle_neck, diag_mask=True")
        if attribute_dict is None:
            raise NotImplementedError("attribute_dict is required (main.py:580, :623)")
        dev = _default_device()
        self.pff_classifier = PositionwiseFeedForward([d_model, 1], reshape=True, use_bias=True)
        self.node_embedding = node_embedding
        self.encode1 = EncoderLayer(n_head, d_model, d_k, d_v, dropout_mul=0.3, dropout_pff=0.4, diag_mask=diag_mask,
                                    bottle_neck=bottle_neck)
        self.encode2 = EncoderLayer(n_head, d_model, d_k, d_v, dropout_mul=0.3, dropout_pff=0.4, diag_mask=diag_mask,
                                    bottle_neck=bottle_neck)       # dead (Modules.py:272 is commented out)
        self.diag_mask_flag = diag_mask
        self.layer_norm1 = nn.LayerNorm(d_model)
        self.layer_norm2 = nn.LayerNorm(d_model)
        self.next_w = FeedForward([bottle_neck, bottle_neck]).to(dev)
        table = torch.from_numpy(np.asarray(attribute_dict, dtype=np.float32)).to(dev)
        self.attribute_dict_embedding = nn.Embedding(len(table), 1, padding_idx=0)
        self.attribute_dict_embedding.weight = nn.Parameter(table)
        self.attribute_dict_embedding.weight.requires_grad = False
        self.attribute_nn = nn.Linear(table.shape[-1], bottle_neck)
        self.attribute_dict = self.attribute_dict_embedding

    # Node ids are validated on the device (ids outside [0, N] are flagged and read as the padding id, so no kernel indexes out
    # of bounds); with check_ids the flag is read back after every call -- one 16-byte device-to-host copy -- and raised as the
    # reference's IndexError.  Bulk callers that issue many forwards back to back (predict.py's sweeps) switch it off and call
    # check_status() once at the end.  Class attribute, so that models pickled by the reference get it too.
    check_ids = True

    # Rows of 9 .. 32 columns train through autograd when this is set (model.long_row_training = True): model(x) in train mode, or with grad
    # enabled and trainable parameters, then runs matcha_forward_long_train / matcha_backward_long -- loss.backward() and torch optimisers, as
    # with the reference.  Off by default: such a call raises NotImplementedError as before.  engine.Trainer, the sampler and the sweeps
    # stay at 8 columns either way.  Class attribute, like check_ids, so that models pickled by the reference get it too.
    long_row_training = False

    def check_status(self):
        self._runtime().check_status("Classifier")

    def deferred_id_check(self):
        """Context manager for bulk callers: ``with model.deferred_id_check(): ...many forwards...`` enqueues the calls without
        the per-call status read-back and raises the reference's IndexError once, at the end of the block."""
        return _DeferredIdCheck(self)

    # ---- runtime plumbing ---------------------------------------------------------------------------
    def __getstate__(self):
        st = self.__dict__.copy()
        st.pop("_rt", None)
        return st

    def _runtime(self) -> _Runtime:
        rt = self.__dict__.get("_rt")
        if rt is None or not rt.still_packed() or rt.device != self.layer_norm1.weight.device:
            rt = _Runtime(self)
            self.__dict__["_rt"] = rt
        return rt

    def _dropout_p(self):
        ne = self.node_embedding
        p_adj = float(ne.dropout.p) if hasattr(ne, "dropout") and ne.dropout is not None else 0.0
        mha, pff = self.encode1.mul_head_attn, self.encode1.pff_n1
        p_fc1 = float(mha.dropout.p) if mha.dropout is not None else 0.0
        p_pff = float(pff.dropout.p) if pff.dropout is not None else 0.0
        return p_adj, p_fc1, p_pff

    def _opts(self, rt: _Runtime, return_recon: bool):
        o = _lib.StepOpts()
        o.training = 1 if self.training else 0
        o.p_drop_adj, o.p_drop_fc1, o.p_drop_pff = self._dropout_p()
        o.alpha, o.beta = 1.0, 1.0
        o.random_chrom = 0
        # no autograd graph will be built -> the library may run its fully fused forward and keep nothing for backward
        o.forward_only = 0 if (torch.is_grad_enabled() and any(p.requires_grad for p in rt.live)) else 1
        if rt.mode == 1:
            # the reference draws this from numpy's global generator on EVERY forward, train and eval (Modules.py:192)
            o.random_chrom = int(np.random.choice(np.arange(rt.n_chrom), 1)[0])
        seed_t = None
        if self.training and (o.p_drop_adj > 0 or o.p_drop_fc1 > 0 or o.p_drop_pff > 0):
            rt.seed_counter += 1
            seed_t = torch.full((1,), (int(torch.initial_seed()) * 1000003 + rt.seed_counter) & 0x7FFFFFFFFFFFFFFF,
                                dtype=torch.int64, device=rt.device)
            o.seed = seed_t.data_ptr()
        return o, seed_t

    # ---- the reference's call surface -----------------------------------------------------------------
    def forward(self, x, mask=None, get_outlier=None, return_recon=False):
        """Logits [B, 1] of the hyperedges x [B, L] (reference Modules.py:278-311).  ``mask`` and ``get_outlier`` are accepted and ignored,
        as the reference ignores them; what ``get_outlier`` was for -- the least supported loci of a hyperedge -- is ``locus_scores``."""
        rt = self._runtime()
        x = torch.as_tensor(x).to(device=rt.device, dtype=torch.long)
        if x.dim() != 2:
            raise ValueError("x must be [B, L] node ids (0 = padding)")
        x = x.contiguous()
        if x.shape[1] > _lib.MAX_LONG_L:
            raise ValueError(f"hyperedges wider than {_lib.MAX_LONG_L} are not supported (x has {x.shape[1]} columns)")
        if x.shape[1] > _lib.MAX_L:
            return self._forward_long(x, rt, return_recon)
        opts, seed_t = self._opts(rt, return_recon)
        logits, recon = _ClassifierFn.apply(x, rt, opts, seed_t, *rt.live)
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.forward")          # IndexError for ids outside [0, N], like the reference's nn.Embedding
        return (logits, recon) if return_recon else logits

    def _forward_long(self, x, rt: _Runtime, return_recon: bool):
        """Rows of MAX_L + 1 .. MAX_LONG_L columns (9 .. 32).  Eval mode without an autograd graph: the long forward (matcha_forward_long)
        and its small workspace.  Same surface as the short path -- logits [B, 1], return_recon, check_ids / deferred_id_check, one
        np.random.choice per call in adj mode.  Train mode, or a graph: NotImplementedError unless ``long_row_training`` is set; then
        the training pair behind _ClassifierLongFn (dropout, loss.backward(), a RuntimeError on a second backward)."""
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in rt.live)):
            if not self.long_row_training:
                raise NotImplementedError(
                    f"hyperedges of more than {_lib.MAX_L} nodes are inference-only (x has {x.shape[1]} columns): call model.eval() and "
                    "run the forward under torch.no_grad(), or set model.long_row_training = True to train on them through autograd")
            opts, seed_t = self._opts(rt, return_recon)       # one np.random.choice in adj mode, the dropout seed from rt.seed_counter
            opts.forward_only = 0                             # (train mode under no_grad: the training layout all the same -- dropout lives there)
            logits, recon = _ClassifierLongFn.apply(x, rt, opts, seed_t, *rt.live)
            if self.check_ids and not torch.cuda.is_current_stream_capturing():
                rt.check_status("Classifier.forward")
            return (logits, recon) if return_recon else logits
        opts, _ = self._opts(rt, return_recon)       # eval + no graph: training = 0, forward_only = 1, no seed
        B, L = x.shape
        ws = rt.workspace(B, L, long_rows=True)
        logits = torch.empty(B, dtype=torch.float32, device=rt.device)
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        opts.status = rt.status.data_ptr()
        _lib.check(rt.lib.matcha_forward_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                              _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws), ws.numel(), rt.stream()),
                   "matcha_forward_long")
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.forward")
        logits = logits.view(B, 1)
        return (logits, losses[1:2]) if return_recon else logits

    def locus_scores(self, x, lowest: int = 0):
        """Which locus of a hyperedge does the model support least?  ``LocusScores(logits [B,1], scores [B,L], order)``: ``scores[b, l]`` is
        the reference's per-position output ``pff_classifier((layer_norm1(dynamic) - layer_norm2(static))**2)`` (Modules.py:290-311) of the
        locus in slot l of ``x[b]``, exactly 0 at padding slots, and ``logits[b] = scores[b].sum() / (k + 1e-15)`` -- the bits ``model(x)``
        returns on the long-row chain.  ``order`` (``lowest`` > 0, at most 32; otherwise None) is int64 [B, lowest]: the slots of the row's
        ``lowest`` least supported loci, ascending by score, ties to the lower slot, -1 behind the row's k real loci.

        Every width 2 .. 32, one forward (the layer-by-layer long-row chain at every width and embed_dim, then head_scores_kernel).  Scores
        depend on the batch width L as the logits do: the reference's softmax runs over the padding key slots too (SURVEY.md headline fact
        7), so score a cluster at the width it will be compared at.  Eval mode only, not differentiable; ``check_ids`` /
        ``deferred_id_check`` and the one ``np.random.choice`` per call in adj mode as in ``forward``."""
        rt = self._runtime()
        x = torch.as_tensor(x).to(device=rt.device, dtype=torch.long)
        if x.dim() != 2:
            raise ValueError("x must be [B, L] node ids (0 = padding)")
        x = x.contiguous()
        B, L = x.shape
        if L < 2 or L > _lib.MAX_LONG_L:
            raise ValueError(f"locus_scores takes hyperedges of 2 .. {_lib.MAX_LONG_L} columns (x has {L})")
        lowest = int(lowest)
        if lowest < 0 or lowest > _lib.MAX_LONG_L:
            raise ValueError(f"lowest={lowest} outside 0 .. {_lib.MAX_LONG_L}")
        if self.training:
            raise NotImplementedError("locus_scores is inference-only (the scores of a dropout forward are not kept): call model.eval() first")
        opts, _ = self._opts(rt, False)              # one np.random.choice in adj mode; training = 0, no seed
        opts.forward_only = 1
        opts.status = rt.status.data_ptr()
        ws = rt.workspace(B, L, long_rows=True)
        scores = torch.empty(B, L, dtype=torch.float32, device=rt.device)
        logits = torch.empty(B, dtype=torch.float32, device=rt.device)
        order = torch.empty(B, lowest, dtype=torch.long, device=rt.device) if lowest else None
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        _lib.check(rt.lib.matcha_locus_scores(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                              _lib.ptr(scores), _lib.ptr(logits), lowest, _lib.ptr(order), _lib.ptr(losses), _lib.ptr(ws),
                                              ws.numel(), rt.stream()),
                   "matcha_locus_scores")
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.locus_scores")
        return LocusScores(logits.view(B, 1), scores, order)

    def get_node_embeddings(self, x, return_recon=False):
        """Rows of the node-embedding front end, [B, L, d] (reference Modules.py:252-259).  Inference surface
        (main.py:471 save_embeddings); not differentiable here -- training goes through forward()."""
        rt = self._runtime()
        x = torch.as_tensor(x).to(device=rt.device, dtype=torch.long).contiguous()
        sz_b, len_seq = x.shape
        ids = x.view(-1)
        out = torch.empty(ids.numel(), rt.d, dtype=torch.float32, device=rt.device)
        recon = torch.zeros(1, dtype=torch.float32, device=rt.device)
        ws = None
        if rt.mode == 1:
            np.random.choice(np.arange(rt.n_chrom), 1)      # keep numpy's global stream in step with Modules.py:192
            # (only its size matters -- the adj front end's scratch for sz_b * len_seq ids: past MAX_L columns the long query covers it)
            ws = rt.workspace(sz_b, len_seq, long_rows=len_seq > _lib.MAX_L)
        _lib.check(rt.lib.matcha_node_embeddings(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), _lib.ptr(ids), ids.numel(),
                                                 _lib.ptr(out), _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.ptr(rt.status),
                                                 rt.stream()),
                   "matcha_node_embeddings")
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.get_node_embeddings")
        out = out.view(sz_b, len_seq, -1)
        return (out, recon) if return_recon else out

    def get_embedding(self, x, slf_attn_mask=None, non_pad_mask=None, return_recon=False):
        """(dynamic, static, attn[, recon_loss]) of the encoder in the reference's padded layout (reference Modules.py:261-276):
        dynamic [B,L,d] = encode1's pff_n1 output (zero at padding slots), static [B,L,d] = tanh(next_w(node + attribute)),
        attn [8*B, L, L] head-major like the reference's (index h*B + b; key columns as they stand in x).  The two mask
        arguments are accepted and ignored exactly as far as the reference ignores them: non_pad_mask is recomputed from x, the
        key-pad mask never reaches the softmax (SURVEY.md headline fact 7).  Runs the layer-by-layer kernels (the fused path
        keeps these tensors on chip); inference surface, not differentiable.  Rows of padding QUERIES in ``attn`` are zero
        (the reference computes a softmax there that nothing reads).

        Every width model(x) takes, 2 .. 32 columns.  Rows of 9 .. 32 columns (eval mode only: NotImplementedError in train mode -- their
        dropout lives in the training layout, and no width has a differentiable get_embedding) run the long chain, whose attention kernel
        writes ``attn`` itself, in this layout, once.  ``attn`` holds 32 * B * L**2 bytes -- 32 KB per row at L = 32, 328 MB for 10 000
        rows: chunk the input accordingly (predict.attention_maps does)."""
        rt = self._runtime()
        x = torch.as_tensor(x).to(device=rt.device, dtype=torch.long).contiguous()
        B, L = x.shape
        if L > _lib.MAX_LONG_L:
            raise ValueError(f"hyperedges wider than {_lib.MAX_LONG_L} are not supported (x has {L} columns)")
        if L > _lib.MAX_L:
            return self._get_embedding_long(x, rt, return_recon)
        opts, seed_t = self._opts(rt, return_recon)
        opts.forward_only = 0
        opts.status = rt.status.data_ptr()
        ws = rt.workspace(B, L)
        dyn = torch.empty(B, L, rt.d, dtype=torch.float32, device=rt.device)
        sta = torch.empty_like(dyn)
        praw = torch.empty(B, _lib.N_HEAD, L, L, dtype=torch.float32, device=rt.device)      # filled by a copy of the workspace's P
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        _lib.check(rt.lib.matcha_get_embedding(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                               _lib.ptr(dyn), _lib.ptr(sta), _lib.ptr(praw), _lib.ptr(losses), _lib.ptr(ws), ws.numel(),
                                               rt.stream()),
                   "matcha_get_embedding")
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.get_embedding")
        # ragged probabilities -> the reference's [8B, L, L]: key slot l of a real key reads its compact column, every padding
        # slot reads the shared padding column k_b
        real = x != 0
        k = real.sum(1)
        col = torch.where(real, torch.cumsum(real.long(), 1) - 1, k.unsqueeze(1))                 # [B, L] compact column of slot l
        row = torch.where(real, torch.cumsum(real.long(), 1) - 1, torch.zeros_like(col))          # compact row of a real query slot
        p = praw.gather(3, col.view(B, 1, 1, L).expand(B, _lib.N_HEAD, L, L))                     # columns in slot order
        p = p.gather(2, row.view(B, 1, L, 1).expand(B, _lib.N_HEAD, L, L))                        # rows in slot order
        # rows / columns at or beyond k are never written by the attention kernel (uninitialised workspace bytes, possibly NaN):
        # select, do not multiply
        p = torch.where(real.view(B, 1, L, 1), p, torch.zeros((), dtype=p.dtype, device=p.device))
        attn = p.permute(1, 0, 2, 3).reshape(_lib.N_HEAD * B, L, L)
        if return_recon:
            return dyn, sta, attn, losses[1:2]
        return dyn, sta, attn

    def _get_embedding_long(self, x, rt: _Runtime, return_recon: bool):
        """get_embedding for rows of MAX_L + 1 .. MAX_LONG_L columns: matcha_get_embedding_long on the long forward's workspace.  ``attn`` is
        allocated once and every element of it is written by attn_long_prob_kernel -- no memset, no gather passes."""
        if self.training:
            raise NotImplementedError(
                f"get_embedding on hyperedges of more than {_lib.MAX_L} nodes is inference-only (x has {x.shape[1]} columns): call model.eval() first")
        opts, _ = self._opts(rt, return_recon)       # one np.random.choice in adj mode; training = 0, no seed
        opts.forward_only = 1
        opts.status = rt.status.data_ptr()
        B, L = x.shape
        ws = rt.workspace(B, L, long_rows=True)
        dyn = torch.empty(B, L, rt.d, dtype=torch.float32, device=rt.device)
        sta = torch.empty_like(dyn)
        attn = torch.empty(_lib.N_HEAD * B, L, L, dtype=torch.float32, device=rt.device)
        losses = torch.zeros(3, dtype=torch.float32, device=rt.device)
        _lib.check(rt.lib.matcha_get_embedding_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(x), B, L,
                                                    _lib.ptr(dyn), _lib.ptr(sta), _lib.ptr(attn), _lib.ptr(losses), _lib.ptr(ws), ws.numel(),
                                                    rt.stream()),
                   "matcha_get_embedding_long")
        if self.check_ids and not torch.cuda.is_current_stream_capturing():
            rt.check_status("Classifier.get_embedding")
        if return_recon:
            return dyn, sta, attn, losses[1:2]
        return dyn, sta, attn


class _DeferredIdCheck:
    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        self.had, self.prev = "check_ids" in m.__dict__, m.check_ids
        m.__dict__["check_ids"] = False
        return m

    def __exit__(self, exc_type, exc, tb):
        m = self.model
        if self.had:
            m.__dict__["check_ids"] = self.prev
        else:
            m.__dict__.pop("check_ids", None)
        if exc_type is None and self.prev:
            m.check_status()
        return False


class DataGenerator:
    """Epoch batch server (reference Modules.py:620-681): bucket hyperedges by size, duplicate each bucket until it
    holds more than num_batch_per_iter*batch_size rows, shuffle, and hand out that many rows per size per call,
    wrapping around with a reshuffle.  Host-side numpy, as in the reference; mixed sizes are returned as a
    zero-padded [M, max_size] int64 array instead of a ragged object array (which numpy >= 1.24 rejects)."""

    def __init__(self, edges, edge_weight, batch_size, num_batch_per_iter, min_size=2, max_size=2, flag=False):
        self.batch_size, self.num_batch_per_iter = batch_size, num_batch_per_iter
        self.min_size, self.max_size, self.flag = min_size, max_size, flag
        per = [[] for _ in range(max_size + 1)]
        wts = [[] for _ in range(max_size + 1)]
        for e, w in zip(edges, edge_weight):
            e = np.asarray(e)
            e = e[e != 0]
            per[len(e)].append(e)
            wts[len(e)].append(w)
        self.edges = [None] * (max_size + 1)
        self.edge_weight = [None] * (max_size + 1)
        need = num_batch_per_iter * batch_size
        for k in range(min_size, max_size + 1):
            e = np.asarray(per[k], dtype=np.int64).reshape(-1, k)
            w = np.asarray(wts[k], dtype=np.float32)
            while 0 < len(e) <= need:
                e, w = np.concatenate([e, e]), np.concatenate([w, w])
            self.edges[k], self.edge_weight[k] = e, w
            self.shuffle(k)
        self.pointer = np.zeros(max_size + 1, dtype="int")

    def shuffle(self, k):
        idx = np.random.permutation(len(self.edges[k]))
        self.edges[k], self.edge_weight[k] = self.edges[k][idx], self.edge_weight[k][idx]

    def next_iter(self):
        need = self.num_batch_per_iter * self.batch_size
        out_e, out_w = [], []
        for k in range(self.min_size, self.max_size + 1):
            if len(self.edges[k]) == 0:
                continue
            lo = self.pointer[k]
            self.pointer[k] += need
            e, w = self.edges[k][lo:self.pointer[k]], self.edge_weight[k][lo:self.pointer[k]]
            if self.pointer[k] > len(self.edges[k]):
                self.shuffle(k)
                left = need - len(e)
                self.pointer[k] = left
                e = np.concatenate([e, self.edges[k][:left]])
                w = np.concatenate([w, self.edge_weight[k][:left]])
            out_e.append(np.pad(e, ((0, 0), (0, self.max_size - k))))
            out_w.append(w)
        return np.concatenate(out_e), np.concatenate(out_w)


for _cls in (Classifier, MultipleEmbedding, Wrap_Embedding, SparseEmbedding, TiedAutoEncoder, EncoderLayer, MultiHeadAttention,
             ScaledDotProductAttention, PositionwiseFeedForward, FeedForward, DataGenerator):
    _cls.__module__ = _PUBLIC_MODULE
