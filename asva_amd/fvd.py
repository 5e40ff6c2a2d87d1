"""FVD on the device: the Inception-v1 I3D feature extractor, its video preprocessing, and (from asva_amd.fid) the Fréchet distance.

Mirrors avgen/evaluations/models/pytorch_i3d.py:9-326 (MaxPool3dSamePadding, Unit3D, InceptionModule, InceptionI3d: the architecture
the StyleGAN-V detector `i3d_torchscript.pt` was converted from), avgen/evaluations/fvd/compute_fvd.py (per-frame antialiased bicubic
resize to 224 x 224, values to (-1, 1)) and avgen/evaluations/models/download.py:47-55 (load_i3d_pretrained).

`InceptionI3d` is a parameter holder with the reference module's state-dict layout (`<endpoint>.conv3d.weight`, `<endpoint>.bn.*`,
`Mixed_xx.{b0,b1a,b1b,b2a,b2b,b3b}.*`, `logits.conv3d.{weight,bias}`); the arithmetic runs in libavsd_hip.so.  Every window uses
TensorFlow "same" padding computed from the input size, which is asymmetric for the stride-2 layers: every Unit3D, with its eval-mode
BatchNorm folded into weights and bias at pack time, is one `avsd_conv3d_same_f32` launch that writes straight into its channel slice
of the block's concatenated output; `b1a` and `b2a` of a block are stacked into one launch whose consumers read channel slices of its
output; the pools are `avsd_maxpool3d_same_f32`, in which a padded position counts as 0.0 as in the reference.  There is no concat or
copy kernel.  Activation widths that are not multiples of 32 and feed a convolution (16, 24, 48, 112, 144, and the 528 channels of
Mixed_4e) are zero-padded at pack time so that their consumers take the float4 loader; a zero tap adds fma(0, 0, acc) and changes no
bit.  The stem (cin 3, K = 1029) takes the scalar loader: the run loader written for it measured 2 % slower (profiles/fvd.md).  Everything is f32 on the f32-input matrix cores, in the bf16 and the fp16
build of the library alike, and every output element is one fixed-order chain: a feature row does not depend on the batch or the
chunk it was computed in.

Nothing is ever downloaded: the detector is a path argument or $AVSD_FVD_I3D.  **No I3D archive was available when this was written:
the path is pinned against the reference's own module with seeded weights (tests/i3d_ref.py, tests/golden/fvd); the archive's key
names, the `bn_eps` choice for it, and the claim that `return_features=True` of the archive equals `InceptionI3d.forward`'s
time-averaged logits are unverified, and no FVD of a real clip has been measured.**
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple, Union

import torch

from . import f32net, ops
from .avsync import _RESIZE
from .fid import frechet_distance  # noqa: F401  (the distance FVD uses, re-exported)
from .weights import _Pk

ENV_WEIGHTS = "AVSD_FVD_I3D"
INPUT_SIZE = 224
MIN_FRAMES = 9              # 8 frames leave one temporal position for the [2, 7, 7] average pool
BN_EPS = 1e-5               # pytorch_i3d.py:71
ARCHIVE_BN_EPS = 1e-3       # load_i3d_pretrained's default for a TorchScript archive: see its docstring
NUM_CLASSES = 400
CHUNK = 8                   # clips per pass of compute_fvd_video_features
# activation widths padded with zero channels at pack time (to a multiple of 32: the float4 loader)
_PAD = {16: 32, 24: 32, 48: 64, 112: 128, 144: 160, 528: 544}


def _padded(c: int) -> int:
    return _PAD.get(c, c)


# ---- architecture as data ---------------------------------------------------------------------------------------------------------------
VALID_ENDPOINTS = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b", "Mixed_3c",
                   "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2", "Mixed_5b", "Mixed_5c",
                   "Logits", "Predictions")
STAGE_NAMES = list(VALID_ENDPOINTS[:-2])
# (name, cin, cout, window, stride)
STEM = [("Conv3d_1a_7x7", 3, 64, (7, 7, 7), (2, 2, 2)), ("Conv3d_2b_1x1", 64, 64, (1, 1, 1), (1, 1, 1)),
        ("Conv3d_2c_3x3", 64, 192, (3, 3, 3), (1, 1, 1))]
# (window, stride) of the max pools
POOLS = {"MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)),
         "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)), "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2))}
BRANCH_POOL = ((3, 3, 3), (1, 1, 1))
# (name, cin, [b0, b1a, b1b, b2a, b2b, b3b])
MIXED = [("Mixed_3b", 192, [64, 96, 128, 16, 32, 32]), ("Mixed_3c", 256, [128, 128, 192, 32, 96, 64]),
         ("Mixed_4b", 480, [192, 96, 208, 16, 48, 64]), ("Mixed_4c", 512, [160, 112, 224, 24, 64, 64]),
         ("Mixed_4d", 512, [128, 128, 256, 24, 64, 64]), ("Mixed_4e", 512, [112, 144, 288, 32, 64, 64]),
         ("Mixed_4f", 528, [256, 160, 320, 32, 128, 128]), ("Mixed_5b", 832, [256, 160, 320, 32, 128, 128]),
         ("Mixed_5c", 832, [384, 192, 384, 48, 128, 128])]
ONE, THREE = (1, 1, 1), (3, 3, 3)


def conv_specs() -> list:
    specs = list(STEM)
    for n, cin, (o0, o1a, o1b, o2a, o2b, o3b) in MIXED:
        specs += [(n + ".b0", cin, o0, ONE, ONE), (n + ".b1a", cin, o1a, ONE, ONE), (n + ".b1b", o1a, o1b, THREE, ONE),
                  (n + ".b2a", cin, o2a, ONE, ONE), (n + ".b2b", o2a, o2b, THREE, ONE), (n + ".b3b", cin, o3b, ONE, ONE)]
    return specs


def state_dict_shapes(num_classes: int = NUM_CLASSES, in_channels: int = 3) -> Dict[str, Tuple[int, ...]]:
    """the layout of the reference's InceptionI3d(num_classes, in_channels=in_channels).state_dict()"""
    shapes: Dict[str, Tuple[int, ...]] = {}
    for name, cin, cout, k, _ in conv_specs():
        shapes[name + ".conv3d.weight"] = (cout, in_channels if name == "Conv3d_1a_7x7" else cin, *k)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{leaf}"] = (cout,)
        shapes[name + ".bn.num_batches_tracked"] = ()
    shapes["logits.conv3d.weight"] = (num_classes, 1024, 1, 1, 1)
    shapes["logits.conv3d.bias"] = (num_classes,)
    return shapes


def same_pad(size: int, k: int, s: int) -> Tuple[int, int]:
    """TensorFlow "same" padding of one axis -> (front, back); the output is ceil(size / s) (pytorch_i3d.py:73-95)"""
    return ops.same_pad(size, k, s)


# ---- packing (pure torch, float64 fold) -------------------------------------------------------------------------------------------------
def _fold(sd, spec, bn_eps: float, cin_pad: int = 0, cout_pad: int = 0) -> _Pk:
    """Unit3D -> one launch: weight * bn scale re-laid [cout][kt][kh][kw][cin] (tap-major, cin-minor), rows padded with zeros to a
    multiple of 4 floats; `cin_pad` / `cout_pad` widen the layer with zero input channels / zero output channels (bias 0: ReLU gives 0)"""
    name, cin, cout, k, s = spec
    w = sd[name + ".conv3d.weight"]
    cin = w.shape[1] if name == "Conv3d_1a_7x7" else cin
    if tuple(w.shape) != (cout, cin, *k):
        raise ValueError(f"{name}.conv3d.weight is {tuple(w.shape)}, expected {(cout, cin, *k)}")
    scale, bias = f32net.bn_affine(*(sd[f"{name}.bn.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var")), bn_eps)
    return f32net.fold_conv(w, scale, bias, taps=k, stride=s, cin_pad=cin_pad, cout_pad=cout_pad)


_stack = f32net.stack_1x1


def fold_network(sd, bn_eps: float = BN_EPS) -> _Pk:
    specs = {s[0]: s for s in conv_specs()}

    def f(name, **kw):
        return _fold(sd, specs[name], bn_eps, **kw)

    stem = [f(s[0]) for s in STEM]
    blocks = []
    for n, cin, (o0, o1a, o1b, o2a, o2b, o3b) in MIXED:
        width = o0 + o1b + o2b + o3b
        b = _Pk(b0=f(n + ".b0", cin_pad=_padded(cin)),
                red=_stack([f(n + ".b1a", cin_pad=_padded(cin), cout_pad=_padded(o1a)),
                            f(n + ".b2a", cin_pad=_padded(cin), cout_pad=_padded(o2a))]),
                b1b=f(n + ".b1b", cin_pad=_padded(o1a)), b2b=f(n + ".b2b", cin_pad=_padded(o2a)),
                # a block whose width is padded carries the zero channels at the end of its last branch
                b3b=f(n + ".b3b", cin_pad=_padded(cin), cout_pad=o3b + _padded(width) - width))
        b.split, b.width = _padded(o1a), width
        blocks.append(b)
    w = sd["logits.conv3d.weight"].detach().float()
    if w.dim() != 5 or tuple(w.shape[1:]) != (1024, 1, 1, 1):
        raise ValueError(f"logits.conv3d.weight is {tuple(w.shape)}, expected (num_classes, 1024, 1, 1, 1)")
    return _Pk(stem=stem, blocks=blocks, logits_w=w.reshape(w.shape[0], 1024).contiguous(),
               logits_b=sd["logits.conv3d.bias"].detach().float().contiguous())


# ---- the network as a sequence of launches; `be` supplies conv / pool / mean / linear (the device library; torch ops in the CPU test) --
class _Hip(f32net._HipBase):
    @staticmethod
    def conv(x, layer, out=None):
        return ops.conv3d_same_f32(x, layer.w, layer.taps, layer.stride, out=out, bias=layer.bias, relu=True)

    pool = staticmethod(ops.maxpool3d_same_f32)


def _run_block(b: _Pk, x: torch.Tensor, be) -> torch.Tensor:
    n, t, h, w, _ = x.shape
    c0, c1, c2, c3 = b.b0.cout, b.b1b.cout, b.b2b.cout, b.b3b.cout
    out = be.empty((n, t, h, w, c0 + c1 + c2 + c3), x)
    be.conv(x, b.b0, out[..., 0:c0])
    r = be.conv(x, b.red)                                                       # [b1a | b2a], each padded to a multiple of 32
    be.conv(r[..., 0:b.split], b.b1b, out[..., c0:c0 + c1])
    be.conv(r[..., b.split:], b.b2b, out[..., c0 + c1:c0 + c1 + c2])
    be.conv(be.pool(x, *BRANCH_POOL), b.b3b, out[..., c0 + c1 + c2:])
    return out


def run_network(pk: _Pk, x: torch.Tensor, be=_Hip, stages: Optional[dict] = None) -> torch.Tensor:
    """x [n, t, h, w, 3] channels-last in (-1, 1) -> (n, num_classes): the logits averaged over the temporal positions that the
    [2, 7, 7] average pool leaves.  `stages`, if a dict, receives the output of every endpoint of STAGE_NAMES (channels-last, without
    the zero channels of the padding)."""
    def mark(name, y, width=None):
        if stages is not None:
            stages[name] = y if width is None or width == y.shape[-1] else y[..., :width]
        return y

    s = pk.stem
    y = mark("Conv3d_1a_7x7", be.conv(x, s[0]))
    y = mark("MaxPool3d_2a_3x3", be.pool(y, *POOLS["MaxPool3d_2a_3x3"]))
    y = mark("Conv3d_2b_1x1", be.conv(y, s[1]))
    y = mark("Conv3d_2c_3x3", be.conv(y, s[2]))
    y = mark("MaxPool3d_3a_3x3", be.pool(y, *POOLS["MaxPool3d_3a_3x3"]))
    for (name, _, _), b in zip(MIXED, pk.blocks):
        if name == "Mixed_4b":
            y = mark("MaxPool3d_4a_3x3", be.pool(y, *POOLS["MaxPool3d_4a_3x3"]))
        if name == "Mixed_5b":
            y = mark("MaxPool3d_5a_2x2", be.pool(y, *POOLS["MaxPool3d_5a_2x2"]))
        y = mark(name, _run_block(b, y, be), b.width)
    n, t, h, w, c = y.shape
    if (h, w) != (7, 7) or t < 2:
        raise ValueError(f"the last block is {t} x {h} x {w}: the [2, 7, 7] average pool needs 7 x 7 and at least 2 temporal positions")
    # AvgPool3d([2, 7, 7], stride 1): window i of a sample is the 98 contiguous rows of temporal positions i and i + 1
    if t == 2:
        pooled = be.mean(y).view(n, 1, c)
    else:
        pooled = be.empty((n, t - 1, c), y)
        for i in range(n):
            for j in range(t - 1):
                be.mean(y[i, j:j + 2].view(1, 98, c), pooled[i, j:j + 1])
    logits = be.linear(pooled.reshape(n * (t - 1), c), pk.logits_w, pk.logits_b).view(n, t - 1, -1)
    return be.mean(logits)                                                      # logits.mean(dim=2) of the reference's NCT layout


# ---- the module -------------------------------------------------------------------------------------------------------------------------
class InceptionI3d(f32net.F32Net):
    """pytorch_i3d.py:137-326 as a parameter holder.  Parameters are created uninitialised: load a state dict.  `bn_eps` is the
    epsilon of every BatchNorm (the reference's module: 1e-5)."""

    VALID_ENDPOINTS = VALID_ENDPOINTS

    def __init__(self, num_classes: int = NUM_CLASSES, spatial_squeeze: bool = True, final_endpoint: str = "Logits",
                 name: str = "inception_i3d", in_channels: int = 3, dropout_keep_prob: float = 0.5, bn_eps: float = BN_EPS):
        super().__init__()
        if final_endpoint not in self.VALID_ENDPOINTS:
            raise ValueError("Unknown final endpoint %s" % final_endpoint)
        if final_endpoint != "Logits":
            raise NotImplementedError(f"only the whole network is built (final_endpoint='Logits'), got {final_endpoint!r}")
        if not spatial_squeeze:
            raise NotImplementedError("only spatial_squeeze=True is built: the evaluation uses (B, num_classes) features")
        if in_channels != 3:
            raise NotImplementedError("only in_channels=3 is built: the stem reads the RGB output of preprocess_videos")
        self.num_classes, self.bn_eps, self.name = int(num_classes), float(bn_eps), name
        f32net.declare(self, state_dict_shapes(self.num_classes, in_channels))
        self.eval()

    def _fold(self, state_dict) -> _Pk:
        return fold_network(state_dict, self.bn_eps)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, timesteps=None, rescale: bool = False, resize: bool = False, return_features: bool = True,
                stages: Optional[dict] = None) -> torch.Tensor:
        """x (B, 3, T, H, W) in (-1, 1) (the reference feeds 224 x 224) -> (B, num_classes).  `rescale=False, resize=False,
        return_features=True` is what compute_fvd_video_features passes to the detector archive; the archive's own rescaling and
        resizing are not built.  `timesteps` is accepted and unused, as in the reference."""
        if rescale or resize:
            raise NotImplementedError("rescale=True / resize=True of the detector archive are not built: pass the output of "
                                      "preprocess_videos with rescale=False, resize=False")
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError(f"input must be (B, 3, T, H, W), got {tuple(x.shape)}")
        b, _, t, h, w = x.shape
        if t < MIN_FRAMES:
            raise ValueError(f"a clip of {t} frames is too short: I3D needs at least {MIN_FRAMES} frames (two temporal positions "
                             "must reach the [2, 7, 7] average pool)")
        if not (193 <= h <= 224 and 193 <= w <= 224):
            raise ValueError(f"input {h} x {w} does not end at 7 x 7 before the average pool: the spatial size must be 193 .. 224")
        xc = x.float().permute(0, 2, 3, 4, 1).contiguous()                      # no copy for the output of preprocess_videos
        return run_network(self.pack(x.device), xc, stages=stages)


def load_i3d_pretrained(device: Union[str, torch.device] = "cpu",
                        weights: Union[None, str, os.PathLike, Dict[str, torch.Tensor]] = None,
                        bn_eps: Optional[float] = None) -> InceptionI3d:
    """download.py:47-55, without its download: `weights` is the path of the StyleGAN-V detector `i3d_torchscript.pt` (a TorchScript
    archive: opened with torch.jit.load on the CPU, only its state_dict() is used), the path of a plain checkpoint
    (torch.load(weights_only=True)), or a loaded state dict; without it the environment variable AVSD_FVD_I3D names the file.

    `bn_eps`: the reference's module says 1e-5 (pytorch_i3d.py:71), and that is the default for a plain checkpoint or a state dict.  The
    TensorFlow network the archive was converted from most likely used 1e-3, so a TorchScript archive defaults to 1e-3.  That choice
    is UNVERIFIED — no archive was available — as are the archive's key names; pass bn_eps to override."""
    weights = f32net.resolve_checkpoint(weights, ENV_WEIGHTS, "I3D detector",
                                        "path of i3d_torchscript.pt or of a checkpoint, or a state dict")
    archive = False
    if not isinstance(weights, dict):
        path = weights
        import zipfile

        archive = zipfile.is_zipfile(path) and any(n.endswith("constants.pkl") or "/code/" in n for n in zipfile.ZipFile(path).namelist())
        if archive:
            weights = dict(torch.jit.load(path, map_location="cpu").state_dict())
        else:
            weights = torch.load(path, map_location="cpu", weights_only=True)
    if bn_eps is None:
        bn_eps = ARCHIVE_BN_EPS if archive else BN_EPS
    net = InceptionI3d(int(weights["logits.conv3d.weight"].shape[0]) if "logits.conv3d.weight" in weights else NUM_CLASSES, bn_eps=bn_eps)
    net.load_state_dict(weights)
    return net.to(device)


# ---- preprocessing and features (compute_fvd.py) ----------------------------------------------------------------------------------------
def preprocess_videos(videos: torch.Tensor, sequence_length: Optional[int] = None) -> torch.Tensor:
    """compute_fvd.py preprocess_videos: BCTHW in [0, 1] -> (B, 3, T, 224, 224) in (-1, 1): optional temporal crop, per-frame
    antialiased bicubic resize (the centre crop to the same size is a no-op), then (v - 0.5) / 0.5, which rounds as the reference's
    v * 2 - 1 does.  The result is a BCTHW VIEW of channels-last memory [b][t][h][w][3], which the network reads without a copy."""
    if videos.dim() != 5 or videos.shape[1] != 3:
        raise ValueError(f"videos must be (B, 3, T, H, W), got {tuple(videos.shape)}")
    if sequence_length is not None:
        if not 0 < sequence_length <= videos.shape[2]:
            raise ValueError(f"sequence_length {sequence_length} exceeds the {videos.shape[2]} frames of the clips")
        videos = videos[:, :, :sequence_length]
    b, _, t, h, w = videos.shape
    frames = videos.float().permute(0, 2, 1, 3, 4).reshape(b * t, 3, h, w).contiguous()
    ytab, xtab = _RESIZE.get(frames.device, h, w, INPUT_SIZE)
    out = ops.resize_aa_normalize_f32(frames, ytab, xtab, INPUT_SIZE, INPUT_SIZE, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    return out.view(b, t, INPUT_SIZE, INPUT_SIZE, 3).permute(0, 4, 1, 2, 3)


@torch.no_grad()
def compute_fvd_video_features(videos: torch.Tensor, net: InceptionI3d, chunk: int = CHUNK) -> torch.Tensor:
    """compute_fvd.py compute_fvd_video_features: videos BCTHW in [0, 1] -> (B, num_classes), `chunk` clips at a time.  A row of the
    result does not depend on the batch or the chunk it sat in."""
    if chunk < 1:
        raise ValueError("chunk must be positive")
    if videos.dim() != 5:
        raise ValueError(f"videos must be (B, 3, T, H, W), got {tuple(videos.shape)}")
    parts = [net(preprocess_videos(videos[i:i + chunk]), rescale=False, resize=False, return_features=True)
             for i in range(0, videos.shape[0], chunk)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)
