"""FID on the device: the pytorch-fid Inception-v3 feature extractor, its preprocessing, and the Fréchet distance.

Mirrors avgen/evaluations/models/inception_v3.py (torchvision's Inception3(num_classes=1008, aux_logits=False) with the four patched
block classes: average pools that do not count padded positions, and the max pool of Mixed_7c), avgen/evaluations/fid/compute_fid.py
(antialiased bicubic resize to 229 x 229, values to (-1, 1)) and avgen/evaluations/dists.py (frechet_distance).

`InceptionV3` is a parameter holder with torchvision's state-dict layout (`<name>.conv.weight`, `<name>.bn.*`, `fc.*`); the arithmetic
runs in libavsd_hip.so.  Every BasicConv2d, with its eval-mode BatchNorm (eps 1e-3) folded into weights and bias at pack time, is one
`avsd_convnd_ld_f32` launch that writes straight into its channel slice of the block's concatenated output; the 1 x 1 convolutions
of a block whose results only feed further convolutions are stacked into one launch, and their consumers read channel slices of its
output.  The three kinds of 3 x 3 pool are `avsd_pool3_hw_f32`.  There is no concat or copy kernel.  The 48- and 80-channel activations
are zero-padded to 64 and 96 channels at pack time so that their consumers take the float4 loader; a zero tap adds fma(0, 0, acc) and
changes no bit.  Everything is f32 on the f32-input matrix cores, in the bf16 and the fp16 build of the library alike, and every output
element is one fixed-order chain: a feature row does not depend on the batch or the chunk it was computed in.

Nothing is ever downloaded: the checkpoint (pytorch-fid's pt_inception-2015-12-05-*.pth) is a path argument or $AVSD_FID_INCEPTION.
No such checkpoint was available when this was written: the path is pinned against a plain-torch restatement with seeded weights
(tests/inception_ref.py, tests/golden/fid), the key names are torchvision's layout taken on trust, and no FID of a real clip has
been measured.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import f32net, ops
from .avsync import _RESIZE
from .weights import _Pk

ENV_WEIGHTS = "AVSD_FID_INCEPTION"
INPUT_SIZE = 229            # the reference's own number (compute_fid.py:11), not Inception's usual 299
BN_EPS = 1e-3
NUM_CLASSES = 1008
CHUNK = 96                  # images per pass of compute_fid_image_features: eight 12-frame clips
_PAD = {48: 64, 80: 96}     # activation widths padded with zero channels at pack time (a multiple of 32: the float4 loader)


# ---- architecture as data: (name, cin, cout, (kh, kw), stride, (ph, pw)) ----------------------------------------------------------------
def _c(name, cin, cout, k=1, s=1, p=0):
    k = (k, k) if isinstance(k, int) else k
    p = (p, p) if isinstance(p, int) else p
    return (name, cin, cout, k, s, p)


STEM = [_c("Conv2d_1a_3x3", 3, 32, 3, 2), _c("Conv2d_2a_3x3", 32, 32, 3), _c("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
        _c("Conv2d_3b_1x1", 64, 80), _c("Conv2d_4a_3x3", 80, 192, 3)]


def _block_a(n, cin, pf):
    return [_c(n + ".branch1x1", cin, 64), _c(n + ".branch5x5_1", cin, 48), _c(n + ".branch5x5_2", 48, 64, 5, 1, 2),
            _c(n + ".branch3x3dbl_1", cin, 64), _c(n + ".branch3x3dbl_2", 64, 96, 3, 1, 1), _c(n + ".branch3x3dbl_3", 96, 96, 3, 1, 1),
            _c(n + ".branch_pool", cin, pf)]


def _block_b(n, cin):
    return [_c(n + ".branch3x3", cin, 384, 3, 2), _c(n + ".branch3x3dbl_1", cin, 64), _c(n + ".branch3x3dbl_2", 64, 96, 3, 1, 1),
            _c(n + ".branch3x3dbl_3", 96, 96, 3, 2)]


def _block_c(n, cin, c7):
    return [_c(n + ".branch1x1", cin, 192), _c(n + ".branch7x7_1", cin, c7), _c(n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
            _c(n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0)), _c(n + ".branch7x7dbl_1", cin, c7),
            _c(n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)), _c(n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)),
            _c(n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)), _c(n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)),
            _c(n + ".branch_pool", cin, 192)]


def _block_d(n, cin):
    return [_c(n + ".branch3x3_1", cin, 192), _c(n + ".branch3x3_2", 192, 320, 3, 2), _c(n + ".branch7x7x3_1", cin, 192),
            _c(n + ".branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), _c(n + ".branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
            _c(n + ".branch7x7x3_4", 192, 192, 3, 2)]


def _block_e(n, cin):
    return [_c(n + ".branch1x1", cin, 320), _c(n + ".branch3x3_1", cin, 384), _c(n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
            _c(n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)), _c(n + ".branch3x3dbl_1", cin, 448),
            _c(n + ".branch3x3dbl_2", 448, 384, 3, 1, 1), _c(n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)),
            _c(n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)), _c(n + ".branch_pool", cin, 192)]


# (block name, kind, its convolutions); kind E1 pools with an average, E2 with a maximum (inception_v3.py:289, :324)
BLOCKS = [("Mixed_5b", "A", _block_a("Mixed_5b", 192, 32)), ("Mixed_5c", "A", _block_a("Mixed_5c", 256, 64)),
          ("Mixed_5d", "A", _block_a("Mixed_5d", 288, 64)), ("Mixed_6a", "B", _block_b("Mixed_6a", 288)),
          ("Mixed_6b", "C", _block_c("Mixed_6b", 768, 128)), ("Mixed_6c", "C", _block_c("Mixed_6c", 768, 160)),
          ("Mixed_6d", "C", _block_c("Mixed_6d", 768, 160)), ("Mixed_6e", "C", _block_c("Mixed_6e", 768, 192)),
          ("Mixed_7a", "D", _block_d("Mixed_7a", 768)), ("Mixed_7b", "E1", _block_e("Mixed_7b", 1280)),
          ("Mixed_7c", "E2", _block_e("Mixed_7c", 2048))]
STAGE_NAMES = ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2"] + \
    [b[0] for b in BLOCKS]
# the reference's output blocks end after these stages (inception_v3.py:69-109)
_BLOCK_END = {0: "maxpool1", 1: "maxpool2", 2: "Mixed_6e", 3: "Mixed_7c"}


def conv_specs() -> list:
    return STEM + [c for _, _, convs in BLOCKS for c in convs]


def state_dict_shapes() -> Dict[str, Tuple[int, ...]]:
    """torchvision's Inception3 layout, which the pytorch-fid checkpoint is saved in"""
    shapes: Dict[str, Tuple[int, ...]] = {}
    for name, cin, cout, (kh, kw), _, _ in conv_specs():
        shapes[name + ".conv.weight"] = (cout, cin, kh, kw)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{leaf}"] = (cout,)
        shapes[name + ".bn.num_batches_tracked"] = ()
    shapes["fc.weight"] = (NUM_CLASSES, 2048)
    shapes["fc.bias"] = (NUM_CLASSES,)
    return shapes


# ---- packing (pure torch, float64 fold) ---------------------------------------------------------------------------------------------
def _fold(sd, spec, cin_pad: int = 0, cout_pad: int = 0) -> _Pk:
    """BasicConv2d -> one launch: weight * bn scale re-laid [cout][kh][kw][cin] (tap-major, cin-minor), rows padded with zeros to a
    multiple of 4 floats; `cin_pad` / `cout_pad` widen the layer with zero input channels / zero output channels (bias 0: ReLU gives 0)"""
    name, cin, cout, (kh, kw), s, (ph, pw) = spec
    w = sd[name + ".conv.weight"]
    if tuple(w.shape) != (cout, cin, kh, kw):
        raise ValueError(f"{name}.conv.weight is {tuple(w.shape)}, expected {(cout, cin, kh, kw)}")
    scale, bias = f32net.bn_affine(*(sd[f"{name}.bn.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var")), BN_EPS)
    return f32net.fold_conv(w, scale, bias, taps=(1, kh, kw), stride=(1, s, s), pad=(0, ph, pw), cin_pad=cin_pad, cout_pad=cout_pad)


_stack = f32net.stack_1x1


def fold_network(sd) -> _Pk:
    specs = {s[0]: s for s in conv_specs()}

    def f(name, **kw):
        return _fold(sd, specs[name], **kw)

    stem = [f("Conv2d_1a_3x3"), f("Conv2d_2a_3x3"), f("Conv2d_2b_3x3"), f("Conv2d_3b_1x1", cout_pad=_PAD[80]),
            f("Conv2d_4a_3x3", cin_pad=_PAD[80])]
    blocks = []
    for n, kind, _ in BLOCKS:
        g = lambda leaf, **kw: f(f"{n}.{leaf}", **kw)      # noqa: E731
        if kind == "A":
            b = _Pk(b1=g("branch1x1"), red=_stack([g("branch5x5_1", cout_pad=_PAD[48]), g("branch3x3dbl_1")]),
                    b5=g("branch5x5_2", cin_pad=_PAD[48]), d2=g("branch3x3dbl_2"), d3=g("branch3x3dbl_3"), bp=g("branch_pool"))
        elif kind == "B":
            b = _Pk(b3=g("branch3x3"), d1=g("branch3x3dbl_1"), d2=g("branch3x3dbl_2"), d3=g("branch3x3dbl_3"))
        elif kind == "C":
            b = _Pk(b1=g("branch1x1"), red=_stack([g("branch7x7_1"), g("branch7x7dbl_1")]), s2=g("branch7x7_2"), s3=g("branch7x7_3"),
                    d2=g("branch7x7dbl_2"), d3=g("branch7x7dbl_3"), d4=g("branch7x7dbl_4"), d5=g("branch7x7dbl_5"), bp=g("branch_pool"))
        elif kind == "D":
            b = _Pk(red=_stack([g("branch3x3_1"), g("branch7x7x3_1")]), b2=g("branch3x3_2"), s2=g("branch7x7x3_2"), s3=g("branch7x7x3_3"),
                    s4=g("branch7x7x3_4"))
        else:
            b = _Pk(b1=g("branch1x1"), red=_stack([g("branch3x3_1"), g("branch3x3dbl_1")]), a2a=g("branch3x3_2a"), a2b=g("branch3x3_2b"),
                    d2=g("branch3x3dbl_2"), d3a=g("branch3x3dbl_3a"), d3b=g("branch3x3dbl_3b"), bp=g("branch_pool"))
        b.kind = kind
        blocks.append(b)
    fc_w = sd["fc.weight"].detach().float().contiguous()
    if tuple(fc_w.shape) != (NUM_CLASSES, 2048):
        raise ValueError(f"fc.weight is {tuple(fc_w.shape)}, expected {(NUM_CLASSES, 2048)}")
    return _Pk(stem=stem, blocks=blocks, fc_w=fc_w, fc_b=sd["fc.bias"].detach().float().contiguous())


# ---- the network as a sequence of launches; `be` supplies conv / pool / mean / linear (the device library; torch ops in the CPU test) --
class _Hip(f32net._HipBase):
    @staticmethod
    def conv(x, layer, out=None):
        return ops.convnd_ld_f32(x, layer.w, layer.taps, layer.stride, layer.pad, out=out, bias=layer.bias, relu=True)

    pool = staticmethod(ops.pool3_hw_f32)


def _out_hw(h, w, layer):
    (_, kh, kw), (_, sh, sw), (_, ph, pw) = layer.taps, layer.stride, layer.pad
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def _run_block(b: _Pk, x: torch.Tensor, be) -> torch.Tensor:
    n, _, h, w, cin = x.shape
    k = b.kind
    if k == "A":
        out = be.empty((n, 1, h, w, 64 + 64 + 96 + b.bp.cout), x)
        be.conv(x, b.b1, out[..., 0:64])
        t = be.conv(x, b.red)                                               # [5x5_1 (48 -> 64 wide) | 3x3dbl_1 (64)]
        be.conv(t[..., 0:64], b.b5, out[..., 64:128])
        be.conv(be.conv(t[..., 64:128], b.d2), b.d3, out[..., 128:224])
        be.conv(be.pool(x, "avg", 1, 1), b.bp, out[..., 224:])
    elif k == "B":
        ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        out = be.empty((n, 1, ho, wo, 384 + 96 + cin), x)
        be.conv(x, b.b3, out[..., 0:384])
        be.conv(be.conv(be.conv(x, b.d1), b.d2), b.d3, out[..., 384:480])
        be.pool(x, "max", 2, 0, out=out[..., 480:])
    elif k == "C":
        c7 = b.s2.cin
        out = be.empty((n, 1, h, w, 768), x)
        be.conv(x, b.b1, out[..., 0:192])
        t = be.conv(x, b.red)                                               # [7x7_1 | 7x7dbl_1]
        be.conv(be.conv(t[..., 0:c7], b.s2), b.s3, out[..., 192:384])
        be.conv(be.conv(be.conv(be.conv(t[..., c7:], b.d2), b.d3), b.d4), b.d5, out[..., 384:576])
        be.conv(be.pool(x, "avg", 1, 1), b.bp, out[..., 576:])
    elif k == "D":
        ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        out = be.empty((n, 1, ho, wo, 320 + 192 + cin), x)
        t = be.conv(x, b.red)                                               # [3x3_1 | 7x7x3_1]
        be.conv(t[..., 0:192], b.b2, out[..., 0:320])
        be.conv(be.conv(be.conv(t[..., 192:], b.s2), b.s3), b.s4, out[..., 320:512])
        be.pool(x, "max", 2, 0, out=out[..., 512:])
    else:
        out = be.empty((n, 1, h, w, 2048), x)
        be.conv(x, b.b1, out[..., 0:320])
        t = be.conv(x, b.red)                                               # [3x3_1 (384) | 3x3dbl_1 (448)]
        be.conv(t[..., 0:384], b.a2a, out[..., 320:704])
        be.conv(t[..., 0:384], b.a2b, out[..., 704:1088])
        u = be.conv(t[..., 384:], b.d2)
        be.conv(u, b.d3a, out[..., 1088:1472])
        be.conv(u, b.d3b, out[..., 1472:1856])
        be.conv(be.pool(x, "avg" if k == "E1" else "max", 1, 1), b.bp, out[..., 1856:])
    return out


def run_network(pk: _Pk, x: torch.Tensor, last_block: int = 3, be=_Hip, stages: Optional[dict] = None) -> Dict[int, torch.Tensor]:
    """x [n, 1, h, w, 3] channels-last in (-1, 1) -> {block index: output}: blocks 0 - 2 channels-last maps [n, 1, h, w, c], block 3
    (n, 2048), block 4 (n, 1008).  `stages`, if a dict, receives the output of every stage of STAGE_NAMES (channels-last)."""
    outs: Dict[int, torch.Tensor] = {}

    def mark(name, y):
        if stages is not None:
            stages[name] = y[..., :80] if name == "Conv2d_3b_1x1" else y       # without the zero channels of the padding
        return y

    s = pk.stem
    y = mark("Conv2d_1a_3x3", be.conv(x, s[0]))
    y = mark("Conv2d_2a_3x3", be.conv(y, s[1]))
    y = mark("Conv2d_2b_3x3", be.conv(y, s[2]))
    y = outs[0] = mark("maxpool1", be.pool(y, "max", 2, 0))
    if last_block >= 1:
        y = mark("Conv2d_3b_1x1", be.conv(y, s[3]))
        y = mark("Conv2d_4a_3x3", be.conv(y, s[4]))
        y = outs[1] = mark("maxpool2", be.pool(y, "max", 2, 0))
    if last_block >= 2:
        for (name, _, _), b in zip(BLOCKS, pk.blocks):
            if name == "Mixed_7a" and last_block < 3:
                break
            y = mark(name, _run_block(b, y, be))
            if name == "Mixed_6e":
                outs[2] = y
    if last_block >= 3:
        y = outs[3] = be.mean(y)                                            # AdaptiveAvgPool2d((1, 1)) + flatten
    if last_block >= 4:
        outs[4] = be.linear(y, pk.fc_w, pk.fc_b)
    return outs


# ---- the module -----------------------------------------------------------------------------------------------------------------------
class InceptionV3(f32net.F32Net):
    """inception_v3.py:16-150.  `output_blocks`: 0 first max pool (64 maps), 1 second max pool (192), 2 Mixed_6e (768), 3 the final
    average pool (B, 2048), 4 the classifier (B, 1008).  Parameters are created uninitialised: load a state dict."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3, 1000: 4}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), use_fid_inception: bool = True):
        super().__init__()
        if not use_fid_inception:
            raise NotImplementedError("only the FID variant of Inception-v3 is built (use_fid_inception=True); torchvision's own "
                                      "pretrained network is not")
        self.output_blocks = sorted(int(b) for b in output_blocks)
        if not self.output_blocks or self.output_blocks[0] < 0 or self.output_blocks[-1] > 4:
            raise ValueError(f"output_blocks must be indices 0 .. 4, got {tuple(output_blocks)}")
        self.last_needed_block = self.output_blocks[-1]
        f32net.declare(self, state_dict_shapes())
        self.eval()

    def _fold(self, state_dict) -> _Pk:
        return fold_network(state_dict)

    @torch.no_grad()
    def forward(self, inp: torch.Tensor, stages: Optional[dict] = None) -> List[torch.Tensor]:
        """inp (B, 3, H, W) in (-1, 1) (the reference feeds 229 x 229) -> the requested block outputs, ascending by index"""
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError(f"input must be (B, 3, H, W), got {tuple(inp.shape)}")
        if min(inp.shape[2], inp.shape[3]) < 75:
            raise ValueError(f"input {tuple(inp.shape[2:])} is too small: Inception-v3 needs at least 75 x 75 pixels")
        b, _, h, w = inp.shape
        x = inp.float().permute(0, 2, 3, 1).contiguous().view(b, 1, h, w, 3)      # no copy for the output of preprocess_images
        outs = run_network(self.pack(inp.device), x, self.last_needed_block, stages=stages)
        res = []
        for i in self.output_blocks:
            y = outs[i]
            res.append(y[:, 0].permute(0, 3, 1, 2) if i <= 2 else y)
        return res


def load_inceptionv3_pretrained(block_ids=(3, 4), use_fid_inception: bool = True,
                                weights: Union[None, str, os.PathLike, Dict[str, torch.Tensor]] = None) -> InceptionV3:
    """inception_v3.py:331-332, without its download: `weights` is the path of pytorch-fid's checkpoint
    (pt_inception-2015-12-05-*.pth) or a loaded state dict; without it the environment variable AVSD_FID_INCEPTION names the file."""
    net = InceptionV3(tuple(block_ids), use_fid_inception=use_fid_inception)
    weights = f32net.resolve_checkpoint(weights, ENV_WEIGHTS, "Inception-v3 checkpoint",
                                        "path of pytorch-fid's pt_inception-2015-12-05-*.pth, or a state dict")
    if not isinstance(weights, dict):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    net.load_state_dict(weights)
    return net


# ---- preprocessing and features (compute_fid.py) --------------------------------------------------------------------------------------
def preprocess_images(images: torch.Tensor) -> torch.Tensor:
    """compute_fid.py:5-18: BCHW in [0, 1] -> (B, 3, 229, 229) in (-1, 1): antialiased bicubic resize (the centre crop to the same size
    is a no-op), then (v - 0.5) / 0.5, which rounds as the reference's v * 2 - 1 does.  The result is a BCHW VIEW of channels-last
    memory, which the network reads without a copy."""
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images must be (B, 3, H, W), got {tuple(images.shape)}")
    frames = images.float().contiguous()
    ytab, xtab = _RESIZE.get(frames.device, frames.shape[2], frames.shape[3], INPUT_SIZE)
    out = ops.resize_aa_normalize_f32(frames, ytab, xtab, INPUT_SIZE, INPUT_SIZE, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    return out.permute(0, 3, 1, 2)


@torch.no_grad()
def compute_fid_image_features(images: torch.Tensor, net: InceptionV3, chunk: int = CHUNK) -> torch.Tensor:
    """compute_fid.py:21-31: images BCHW in [0, 1] -> the first requested block of `net` (block 3: (B, 2048)), `chunk` images at a
    time.  A row of the result does not depend on the batch or the chunk it sat in."""
    if chunk < 1:
        raise ValueError("chunk must be positive")
    if images.dim() != 4:
        raise ValueError(f"images must be (B, 3, H, W), got {tuple(images.shape)}")
    parts = [net(preprocess_images(images[i:i + chunk]))[0] for i in range(0, images.shape[0], chunk)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


# ---- Fréchet distance (dists.py:56-119) -------------------------------------------------------------------------------------------------
def frechet_distance(x1: torch.Tensor, x2: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """d^2 = |mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2)) between the Gaussians fitted to the rows of x1 (n1, d) and x2 (n2, d): CPU
    feature tensors in, a float64 scalar tensor out (`.item()` as the reference's numpy scalar).  float64 torch on the host only.

    The symmetric form: with R = S1^(1/2) from torch.linalg.eigh (negative eigenvalues of rounding clamped to 0), S1 S2 is similar
    to the symmetric positive semi-definite R S2 R, so tr sqrt(S1 S2) = sum_i sqrt(max(lambda_i, 0)) over the eigenvalues of R S2 R.
    Every quantity stays real and finite for rank-deficient covariances too, so neither the reference's singular-product fallback
    (adding `eps` to the diagonals) nor its handling of a complex square root is needed; `eps` is accepted and unused."""
    if x1.dim() != 2 or x2.dim() != 2:
        raise ValueError(f"features must be (n, d) matrices, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    if x1.shape[1] != x2.shape[1]:
        raise ValueError(f"feature widths differ: {x1.shape[1]} and {x2.shape[1]}")
    if x1.shape[0] < 2 or x2.shape[0] < 2:
        raise ValueError(f"a covariance needs at least two samples, got {x1.shape[0]} and {x2.shape[0]}")
    x1, x2 = x1.detach().to("cpu", torch.float64), x2.detach().to("cpu", torch.float64)
    mu1, mu2 = x1.mean(0), x2.mean(0)
    d1, d2 = x1 - mu1, x2 - mu2
    s1, s2 = d1.t() @ d1 / (x1.shape[0] - 1), d2.t() @ d2 / (x2.shape[0] - 1)
    lam, vec = torch.linalg.eigh(s1)
    root = (vec * lam.clamp_min(0.0).sqrt()) @ vec.t()
    m = root @ s2 @ root
    tr_covmean = torch.linalg.eigvalsh((m + m.t()) / 2).clamp_min(0.0).sqrt().sum()
    diff = mu1 - mu2
    return diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2.0 * tr_covmean
