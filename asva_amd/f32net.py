"""What the on-device f32 networks share (fid.py, fvd.py, avsync.py, imagebind_eval.py, text_encoder.py): a parameter holder built from a
table of state-dict shapes, its checked loader, the cached pack into ONE weights.Blob, the float64 BatchNorm fold with the re-layout to
[cout][taps][cin] that the f32 convolution kernels read, the launches every one of them uses, and the pre-LN transformer blocks as a
sequence of those launches (`run_blocks`).  Host-side only: no kernel lives here.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import ops
from .modelio import EpochCounted
from .weights import Blob, _Pk, pack_device


def declare(module: nn.Module, shapes: Dict[str, Sequence[int]]) -> None:
    """the nested nn.Module tree whose state_dict() has the keys and shapes of `shapes`, uninitialised: BatchNorm's running statistics
    are f32 buffers, its num_batches_tracked an int64 zero buffer, everything else an f32 parameter without gradient"""
    for key, shape in shapes.items():
        mod, parts = module, key.split(".")
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        if parts[-1] == "num_batches_tracked":
            mod.register_buffer(parts[-1], torch.zeros(shape, dtype=torch.int64))
        elif parts[-1] in ("running_mean", "running_var"):
            mod.register_buffer(parts[-1], torch.empty(shape, dtype=torch.float32))
        else:
            mod.register_parameter(parts[-1], nn.Parameter(torch.empty(shape, dtype=torch.float32), requires_grad=False))


class F32Net(EpochCounted, nn.Module):
    """A network that computes in f32 only, from weights that `_fold` lays out for the kernels and `pack` keeps in one device blob.
    `_epoch` counts the changes of the parameters (load_state_dict, .to()): a pack made under another count is stale."""

    STRICT_KEYS = True      # load_state_dict(strict=True) refuses tensors the model does not have
    ANY_DTYPE = False       # to() ignores a dtype other than float32 instead of refusing it

    def __init__(self):
        super().__init__()
        self._packed: Optional[_Pk] = None

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    def to(self, *args, **kw):
        """moves to a device; dtype=torch.float32 is accepted, any other dtype refused (ignored under ANY_DTYPE): the network computes
        in f32 only"""
        device, dtype = kw.get("device"), kw.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif isinstance(a, (str, torch.device, int)):
                device = a
        if dtype not in (None, torch.float32) and not self.ANY_DTYPE:
            raise ValueError(f"{type(self).__name__} computes in float32 only, got dtype={dtype}")
        if device is not None:
            super().to(device)
        return self

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """every tensor of the model must be there (BatchNorm's num_batches_tracked aside) and have its shape; values are converted to
        the model's dtypes"""
        who = f"{type(self).__name__}.load_state_dict"
        own = super().state_dict()
        missing = [k for k in own if k not in state_dict and not k.endswith("num_batches_tracked")]
        if missing:
            raise KeyError(f"{who}: the checkpoint lacks {len(missing)} tensors, e.g. {missing[:3]}")
        unexpected = [k for k in state_dict if k not in own]
        if strict and self.STRICT_KEYS and unexpected:
            raise KeyError(f"{who}: {len(unexpected)} unexpected tensors, e.g. {unexpected[:3]}")
        for k, p in own.items():
            if k in state_dict and tuple(state_dict[k].shape) != tuple(p.shape):
                raise ValueError(f"{who}: {k!r} is {tuple(state_dict[k].shape)}, expected {tuple(p.shape)}")
        return super().load_state_dict({k: state_dict[k].to(own[k].dtype) if k in state_dict else own[k] for k in own}, strict=True)

    def _fold(self, state_dict) -> _Pk:
        """state_dict -> the tree of attribute bags and lists whose tensors are the kernel layouts"""
        raise NotImplementedError

    def _pack_epoch(self) -> int:
        return self._epoch

    def _after_pack(self, root: _Pk) -> None:
        """what a subclass derives from the views of the finished blob"""

    def pack(self, device=None) -> _Pk:
        """state_dict -> folded f32 kernel layouts inside ONE device blob built by weights.Blob and stamped with the shared pack key;
        cached, repacked after load_state_dict / .to()"""
        device = pack_device(device)
        pk, epoch = self._packed, self._pack_epoch()
        if pk is not None and pk.epoch == epoch and (device is None or pk.blob.device == device):
            return pk
        device = pack_device(device, self.device, ops, f"{type(self).__name__}.pack")
        blob = Blob()
        root = blob.finish(blob.reg_tree(self._fold(super().state_dict())), device)
        self._after_pack(root)
        root.epoch = epoch
        self._packed = root
        return root


# ---- packing (pure torch, float64 fold) ---------------------------------------------------------------------------------------------
def bn_affine(weight, bias, mean, var, eps: float):
    """eval-mode BatchNorm as y = s * x + b, in float64"""
    s = weight.detach().double() / torch.sqrt(var.detach().double() + eps)
    return s, bias.detach().double() - mean.detach().double() * s


def fold_conv(w, scale, bias, *, taps, stride, pad=None, cin_pad: int = 0, cout_pad: int = 0, **extra) -> _Pk:
    """one convolution launch: weight [cout, cin, (kt,) (kh, kw)] * scale[cout] re-laid [cout][kt][kh][kw][cin] (tap-major, cin-minor),
    rows padded with zeros to a multiple of 4 floats, f32.  `scale` / `bias` are float64 [cout] or None; `cin_pad` / `cout_pad` widen the
    layer with zero input channels / zero output channels (bias 0: ReLU gives 0); `extra` joins the layer's attributes"""
    w = w.detach().double()
    cout, cin = w.shape[:2]
    w = w.reshape(cout, cin, *taps)                     # a 2-D (nn.Linear) or 4-D weight gains the axes of its size-1 taps
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1, 1)
    ci, co = max(cin, cin_pad), max(cout, cout_pad)
    full = torch.zeros((co, *taps, ci), dtype=torch.float64, device=w.device)
    full[:cout, ..., :cin] = w.permute(0, 2, 3, 4, 1)
    k = taps[0] * taps[1] * taps[2] * ci
    mat = torch.zeros((co, (k + 3) // 4 * 4), dtype=torch.float32, device=w.device)
    mat[:, :k] = full.reshape(co, k).float()
    b = None
    if bias is not None:
        b = torch.zeros(co, dtype=torch.float32, device=w.device)
        b[:cout] = bias.float()
    layer = _Pk(w=mat, bias=b, taps=tuple(taps), stride=tuple(stride), cin=ci, cout=co, **extra)
    if pad is not None:
        layer.pad = tuple(pad)
    return layer


def stack_1x1(layers: Sequence[_Pk]) -> _Pk:
    """1 x 1 (x 1) convolutions on the same input as ONE launch: weight rows and biases one after the other"""
    a = layers[0]
    assert all(l.taps == (1, 1, 1) and l.cin == a.cin and l.w.shape[1] == a.w.shape[1] for l in layers)
    return _Pk(**dict(a.__dict__, w=torch.cat([l.w for l in layers]), bias=torch.cat([l.bias for l in layers]),
                      cout=sum(l.cout for l in layers)))


# ---- the launches every network uses ------------------------------------------------------------------------------------------------
class _HipBase:
    empty = staticmethod(lambda shape, like: torch.empty(shape, dtype=torch.float32, device=like.device))
    mean = staticmethod(ops.mean_rows_f32)
    linear = staticmethod(ops.linear_f32)
    layernorm = staticmethod(ops.layernorm_f32)
    attention = staticmethod(ops.attention_f32)
    attention_causal = staticmethod(ops.attention_causal_f32)
    gelu = staticmethod(ops.gelu_f32)
    quick_gelu = staticmethod(ops.quick_gelu_f32)


def run_blocks(h: torch.Tensor, blocks: Sequence[_Pk], b: int, seq: int, heads: int, eps: float, *, causal: bool = False, act: str = "gelu",
               be=_HipBase) -> torch.Tensor:
    """pre-LN transformer blocks on h [b * seq, C], eight launches each; `act` names the backend's activation ("gelu": erf, or
    "quick_gelu").  A packed block is n1_g n1_b in_w in_b out_w out_b n2_g n2_b fc1_w fc1_b fc2_w fc2_b [bias_kv], in_w = q | k | v rows.
    A block with a bias_kv pair overwrites the key / value slots of each sequence's LAST row with it (the caller left that row spare),
    which is exactly MultiheadAttention's appended pair"""
    c = h.shape[1]
    attend, activate = be.attention_causal if causal else be.attention, getattr(be, act)
    for w in blocks:
        qkv = be.linear(be.layernorm(h, w.n1_g, w.n1_b, eps), w.in_w, w.in_b)                     # [b * seq, 3 C] = q | k | v
        if hasattr(w, "bias_kv"):
            slot = qkv.view(b, seq, 3 * c)[:, seq - 1, c:]
            slot.copy_(w.bias_kv.expand_as(slot))
        a = attend(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], b, seq, heads)
        h = be.linear(a, w.out_w, w.out_b, res=h)
        m = be.linear(be.layernorm(h, w.n2_g, w.n2_b, eps), w.fc1_w, w.fc1_b)
        h = be.linear(activate(m, out=m), w.fc2_w, w.fc2_b, res=h)
    return h


def resolve_checkpoint(weights, env_name: str, what: str, accepted: str):
    """the `weights` argument of a loader that downloads nothing: a state dict is returned as it is, a path - or, without one, the
    path in the environment variable `env_name` - as a string, after checking that the file exists"""
    if weights is None:
        weights = os.environ.get(env_name) or None
    if weights is None:
        raise FileNotFoundError(f"no {what}: pass weights=<{accepted}> or set the environment variable {env_name}; nothing is "
                                "downloaded here")
    if isinstance(weights, dict):
        return weights
    path = os.fspath(weights)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{what} {path!r} (weights= or ${env_name}) does not exist")
    return path
