"""AVSync scorer: the reference's audio-video synchronisation classifier and the RelSync metric on it, on the device.

Mirrors avsync/models/{audio,video,head,avsync_classifier}.py (an R(2+1)D-18 video network, a 2-D convolutional audio network
on the log-mel spectrogram, a 3-layer FC head) and avgen/evaluations/avsync/compute_avsync.py (preprocessing, raw score, RelSync).
The classes below are parameter holders with the reference's constructor arguments and `state_dict()` layout; the arithmetic
runs in libavsd_hip.so (csrc/avsync.hip): every convolution, with its eval-mode BatchNorm folded into weights, bias and residual
scale at pack time, is one `avsd_convnd_f32` launch.

Everything is f32 on the f32-input matrix cores, in the bf16 and the fp16 build of the library alike: a score must not move with
the storage mode of the clip it judges.  No host synchronisation inside `forward`; all launches go to the current stream.

Also here, what the reference does with the classifier beyond scoring aligned rows, all of it the FC head on a MATRIX of pairs
(csrc/avsync_pairs.hip): `AVSyncClassifier.pair_scores`, the contrastive objective of avsync/models/sync_contrastive_trainer.py
(`AVSyncContrastiveTrainer`, forward values only) and the shift-accuracy evaluation of scripts/avsync_eval.py (`shifted_pairs`,
`shift_accuracy`, `evaluate_shift_accuracy`; tools/avsync_eval.py).

No trained classifier checkpoint was available when this was written: the path is pinned against the reference's modules with
seeded weights (tests/golden/avsync_tiny.pt), and no RelSync value or shift accuracy of a real checkpoint has been measured.
"""
from __future__ import annotations

import os
import random
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import f32net, modelio, ops
from .weights import _Pk

DEFAULT_MODEL_PATH = "checkpoints/avsync/vggss_sync_contrast/ckpts/checkpoint-40000/modules"
AVID_CMA_CHECKPOINT = "./pretrained/AVID-CMA_Audioset_InstX-N1024-PosW-N64-Top32_checkpoint.pth.tar"
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
INPUT_SIZE = 224


# ---- parameter holders -----------------------------------------------------------------------------------------------------------
class _Pretrained(modelio.EpochCounted, nn.Module):
    """config + diffusers directory layout (config.json + diffusion_pytorch_model.bin / .safetensors) for the three sub-networks;
    `_epoch` counts the changes of the parameters: the packed weights of the enclosing classifier follow every one"""

    _config: Dict

    @property
    def config(self) -> Dict:
        return dict(self._config)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, subfolder: Optional[str] = None, use_safetensors: Optional[bool] = None, **_):
        model = cls(**modelio.read_config(pretrained_model_path, subfolder, drop_private=True))
        model.load_state_dict(modelio.read_state_dict(pretrained_model_path, subfolder, use_safetensors=use_safetensors))
        return model.eval()

    def save_pretrained(self, save_directory: str, safe_serialization: bool = False):
        modelio.write_folder(save_directory, {"_class_name": type(self).__name__, **self._config}, self.state_dict(), safe_serialization)

    def _load_avid_cma(self, prefix: str):
        sd = torch.load(AVID_CMA_CHECKPOINT, map_location="cpu")["model"]
        self.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})


def _conv_bn3d(cin, cout, k, stride, pad):
    return nn.Conv3d(cin, cout, k, stride=stride, padding=pad, bias=False), nn.BatchNorm3d(cout)


class _R2Plus1DBlock(nn.Module):
    """(1,3,3) spatial + (3,1,1) temporal convolution, twice, with a residual (video.py:13-44)"""

    def __init__(self, in_planes: int, out_planes: int, stride=(1, 1, 1)):
        super().__init__()
        self.spt_conv1, self.spt_bn1 = _conv_bn3d(in_planes, out_planes, (1, 3, 3), (1, stride[1], stride[2]), (0, 1, 1))
        self.tmp_conv1, self.tmp_bn1 = _conv_bn3d(out_planes, out_planes, (3, 1, 1), (stride[0], 1, 1), (1, 0, 0))
        self.spt_conv2, self.spt_bn2 = _conv_bn3d(out_planes, out_planes, (1, 3, 3), (1, 1, 1), (0, 1, 1))
        self.tmp_conv2, self.out_bn = _conv_bn3d(out_planes, out_planes, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        self.res = in_planes != out_planes or any(s != 1 for s in stride)
        if self.res:
            self.res_conv = nn.Conv3d(in_planes, out_planes, (1, 1, 1), stride=tuple(stride), bias=False)


class VideoR2Plus1DNet(_Pretrained):
    """video.py:47-81: (b, 3, f, h, w) -> (b, 512)"""

    def __init__(self, pretrained: bool = False):
        super().__init__()
        self._config = {"pretrained": pretrained}
        self.conv1 = nn.Sequential(*_conv_bn3d(3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3)))      # + ReLU + max-pool (no parameters)
        self.conv2x = nn.Sequential(_R2Plus1DBlock(64, 64), _R2Plus1DBlock(64, 64))
        self.conv3x = nn.Sequential(_R2Plus1DBlock(64, 128, (2, 2, 2)), _R2Plus1DBlock(128, 128))
        self.conv4x = nn.Sequential(_R2Plus1DBlock(128, 256, (2, 2, 2)), _R2Plus1DBlock(256, 256))
        self.conv5x = nn.Sequential(_R2Plus1DBlock(256, 512, (2, 2, 2)), _R2Plus1DBlock(512, 512))
        self.out_dim = 512
        if pretrained:
            self._load_avid_cma("module.video_model.")


class _Audio2DBlock(nn.Module):
    def __init__(self, in_planes: int, out_planes: int, stride=(1, 1)):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, out_planes, 3, padding=1, stride=stride, bias=False)
        self.bn1 = nn.BatchNorm2d(out_planes)
        self.conv2 = nn.Conv2d(out_planes, out_planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_planes)


class AudioConv2DNet(_Pretrained):
    """audio.py:30-61: (b, 1, n_mel, t) -> (b, 512)"""

    def __init__(self, pretrained: bool = False):
        super().__init__()
        self._config = {"pretrained": pretrained}
        self.conv1 = nn.Sequential(nn.Conv2d(1, 64, 7, padding=3, stride=2, bias=False), nn.BatchNorm2d(64))   # + ReLU
        self.block1 = _Audio2DBlock(64, 64, (2, 2))
        self.block2 = _Audio2DBlock(64, 128, (2, 2))
        self.block3 = _Audio2DBlock(128, 256, (2, 2))
        self.block4 = _Audio2DBlock(256, 512)
        self.out_dim = 512
        if pretrained:
            self._load_avid_cma("module.audio_model.")


class FCHead(_Pretrained):
    """head.py:8-29: Linear - ReLU - Linear - ReLU - Linear on cat(audio, video) (dropout is the identity in eval mode)"""

    def __init__(self, dim: int = 512, out_dim: int = 1, dropout: float = 0.0):
        super().__init__()
        self._config = {"dim": dim, "out_dim": out_dim, "dropout": dropout}
        self.fc = nn.Sequential(nn.Linear(dim * 2, dim), nn.Dropout(dropout), nn.ReLU(), nn.Linear(dim, dim // 2), nn.Dropout(dropout),
                                nn.ReLU(), nn.Linear(dim // 2, out_dim))


# ---- packing: BatchNorm fold + weight re-layout (pure torch, any device: tests/test_avsync_cpu.py applies it with torch ops) -------
def _bn_affine(bn):
    return f32net.bn_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def _triple(v, fill):
    v = tuple(v)
    return v if len(v) == 3 else (fill,) + v


def fold_conv(conv, scale=None, bias=None, relu: bool = False) -> _Pk:
    """one launch of avsd_convnd_f32: weight * scale[cout] re-laid to [cout][taps][cin] (rows padded with zeros to a multiple of 4
    floats), f32; `scale` / `bias` are float64 [cout] or None"""
    if isinstance(conv, nn.Linear):                     # a (1, 1, 1) window over a 1 x 1 x 1 "image"
        taps, stride, pad = (1, 1, 1), (1, 1, 1), (0, 0, 0)
        if conv.bias is not None:
            bias = conv.bias.detach().double() if bias is None else bias + conv.bias.detach().double()
    else:
        taps, stride, pad = _triple(conv.kernel_size, 1), _triple(conv.stride, 1), _triple(conv.padding, 0)
    return f32net.fold_conv(conv.weight, scale, bias, taps=taps, stride=stride, pad=pad, rscale=None, relu=relu)


def fold_video(net: VideoR2Plus1DNet) -> _Pk:
    s, b = _bn_affine(net.conv1[1])
    stages = []
    for stage in (net.conv2x, net.conv3x, net.conv4x, net.conv5x):
        blocks = []
        for blk in stage:
            so, bo = _bn_affine(blk.out_bn)
            # out_bn(main + res) = so * main + so * res + bo: so goes into the last temporal convolution and into the residual
            # projection where there is one; an identity residual is scaled in the epilogue
            d = _Pk(spt1=fold_conv(blk.spt_conv1, *_bn_affine(blk.spt_bn1), relu=True),
                    tmp1=fold_conv(blk.tmp_conv1, *_bn_affine(blk.tmp_bn1), relu=True),
                    spt2=fold_conv(blk.spt_conv2, *_bn_affine(blk.spt_bn2), relu=True),
                    tmp2=fold_conv(blk.tmp_conv2, so, bo, relu=True),
                    res=fold_conv(blk.res_conv, so) if blk.res else None)
            if not blk.res:
                d.tmp2.rscale = so.float().contiguous()
            blocks.append(d)
        stages.append(blocks)
    return _Pk(conv1=fold_conv(net.conv1[0], s, b, relu=True), stages=stages)


def fold_audio(net: AudioConv2DNet) -> _Pk:
    blocks = [[fold_conv(b.conv1, *_bn_affine(b.bn1), relu=True), fold_conv(b.conv2, *_bn_affine(b.bn2), relu=True)]
              for b in (net.block1, net.block2, net.block3, net.block4)]
    return _Pk(conv1=fold_conv(net.conv1[0], *_bn_affine(net.conv1[1]), relu=True), blocks=blocks)


def fold_head(net: FCHead) -> list:
    lins = [m for m in net.fc if isinstance(m, nn.Linear)]
    return [fold_conv(m, relu=i + 1 < len(lins)) for i, m in enumerate(lins)]


# ---- the network as a sequence of launches; `be` supplies conv / maxpool / mean (the device library, or torch ops in the CPU test) --
class _Hip(f32net._HipBase):
    @staticmethod
    def conv(x, layer, res=None):
        return ops.convnd_f32(x, layer.w, layer.taps, layer.stride, layer.pad, bias=layer.bias, res=res,
                              rscale=layer.rscale if res is not None else None, relu=layer.relu)

    maxpool = staticmethod(ops.maxpool_hw_f32)

    @staticmethod
    def half(x, layer, col, bias):
        """x [m, cin] -> x @ layer.w[:, col:col + cin].T + bias, no activation: one column half of a layer that reads a concatenation"""
        m, cin = x.shape
        return ops.convnd_f32(x.view(m, 1, 1, 1, cin), layer.w, (1, 1, 1), (1, 1, 1), (0, 0, 0), bias=bias, w_col=col).view(m, -1)

    @staticmethod
    def pair_head(u, vh, l2, l3):
        return ops.pair_head_f32(u, vh, l2.w, l2.bias, l3.w, l3.bias)

    pair_xent = staticmethod(ops.pair_xent_f32)


def run_video(pk: _Pk, x: torch.Tensor, be=_Hip, stages: Optional[list] = None) -> torch.Tensor:
    """x [n, t, h, w, 3] preprocessed, channels-last -> (n, 512).  `stages`, if a list, receives the output of conv1 (after the
    max-pool) and of the four stages."""
    y = be.maxpool(be.conv(x, pk.conv1))
    if stages is not None:
        stages.append(y)
    for stage in pk.stages:
        for b in stage:
            r = be.conv(y, b.res) if b.res is not None else y
            h = be.conv(be.conv(be.conv(y, b.spt1), b.tmp1), b.spt2)
            y = be.conv(h, b.tmp2, res=r)
        if stages is not None:
            stages.append(y)
    return be.mean(y)


def run_audio(pk: _Pk, x: torch.Tensor, be=_Hip, stages: Optional[list] = None) -> torch.Tensor:
    """x [n, 1, n_mel, t, 1] -> (n, 512)"""
    y = be.conv(x, pk.conv1)
    if stages is not None:
        stages.append(y)
    for c1, c2 in pk.blocks:
        y = be.conv(be.conv(y, c1), c2)
        if stages is not None:
            stages.append(y)
    return be.mean(y)


def run_head(pk: list, audio_emb: torch.Tensor, video_emb: torch.Tensor, be=_Hip) -> torch.Tensor:
    y = torch.cat([audio_emb, video_emb], 1).view(audio_emb.shape[0], 1, 1, 1, -1)
    for layer in pk:
        y = be.conv(y, layer)
    return y.view(y.shape[0], -1)


def run_pair_head(pk: list, audio_emb: torch.Tensor, video_emb: torch.Tensor, be=_Hip) -> torch.Tensor:
    """audio_emb (G, P, D), video_emb (G, Q, D) -> scores (G, P, Q): the head on every (audio p, video q) pair of each group.
    The first layer is linear in cat(a, v): W1 . cat(a_p, v_q) + b1 = Wa . a_p + (Wv . v_q + b1), two launches on the G (P + Q)
    distinct rows; one more launch (avsd_pair_head_f32) does the rest, and neither the (G P Q, 2 D) concatenation nor the
    (G P Q, H1) hidden layer exists.  A head the kernel is not built for (ops.pair_head_supported) goes through `run_head` on the
    materialised pairs: one route per head size, so a score is a function of its pair alone either way."""
    G, P, D = audio_emb.shape
    Q = video_emb.shape[1]
    if len(pk) == 3 and pk[0].cin == 2 * D and pk[0].relu and pk[1].relu and ops.pair_head_supported(D, pk[0].cout, pk[1].cout):
        l1, l2, l3 = pk
        u = be.half(audio_emb.reshape(G * P, D), l1, 0, None).view(G, P, -1)
        vh = be.half(video_emb.reshape(G * Q, D), l1, D, l1.bias).view(G, Q, -1)
        return be.pair_head(u, vh, l2, l3)
    a = audio_emb[:, :, None, :].expand(G, P, Q, D).reshape(G * P * Q, D)
    v = video_emb[:, None, :, :].expand(G, P, Q, D).reshape(G * P * Q, D)
    return run_head(pk, a, v, be)[:, 0].reshape(G, P, Q)


class AVSyncClassifier(f32net.F32Net):
    """avsync_classifier.py:10-33: score = head(audio_encoder(audio), video_encoder(video))[:, 0]"""

    def __init__(self, audio_encoder: AudioConv2DNet, video_encoder: VideoR2Plus1DNet, head: FCHead):
        super().__init__()
        self.audio_encoder = audio_encoder
        self.video_encoder = video_encoder
        self.head = head

    # ---- packing --------------------------------------------------------------------------------------------------------------
    # real torch modules underneath: nn.Module's own loader and .to(); a sub-network loaded or moved on its own counts too
    to = nn.Module.to

    load_state_dict = modelio.EpochCounted.load_state_dict

    def _pack_epoch(self) -> int:
        return self._epoch + sum(m._epoch for m in (self.audio_encoder, self.video_encoder, self.head))

    def _fold(self, state_dict) -> _Pk:
        for m in self.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training:
                raise RuntimeError("AVSyncClassifier.pack: BatchNorm is folded with its running statistics; call .eval() first")
        return _Pk(video=fold_video(self.video_encoder), audio=fold_audio(self.audio_encoder), head=fold_head(self.head))

    # ---- forward --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _audio_cl(audio: torch.Tensor) -> torch.Tensor:
        if audio.dim() != 4 or audio.shape[1] != 1:
            raise ValueError(f"audio must be (b, 1, n_mel, t), got {tuple(audio.shape)}")
        return audio.float().contiguous().view(audio.shape[0], 1, audio.shape[2], audio.shape[3], 1)

    @staticmethod
    def _video_cl(video: torch.Tensor) -> torch.Tensor:
        if video.dim() != 5 or video.shape[1] != 3:
            raise ValueError(f"video must be (b, 3, f, h, w), got {tuple(video.shape)}")
        return video.float().permute(0, 2, 3, 4, 1).contiguous()      # no copy for the output of preprocess_videos

    @torch.no_grad()
    def embed_audio(self, audio: torch.Tensor, stages: Optional[list] = None) -> torch.Tensor:
        return run_audio(self.pack(audio.device).audio, self._audio_cl(audio), stages=stages)

    @torch.no_grad()
    def embed_video(self, video: torch.Tensor, stages: Optional[list] = None) -> torch.Tensor:
        return run_video(self.pack(video.device).video, self._video_cl(video), stages=stages)

    @torch.no_grad()
    def score_embeddings(self, audio_emb: torch.Tensor, video_emb: torch.Tensor) -> torch.Tensor:
        return run_head(self.pack(audio_emb.device).head, audio_emb, video_emb)[:, 0]

    @torch.no_grad()
    def pair_scores(self, audio_emb: torch.Tensor, video_emb: torch.Tensor, be=_Hip) -> torch.Tensor:
        """audio_emb (G, P, D), video_emb (G, Q, D) -> scores (G, P, Q) f32: scores[g, p, q] is the head on (audio p, video q) of
        group g.  Three launches whatever P and Q (`run_pair_head`).  `be`: the backend, as in `run_head`; one that is not the device
        library folds the head from the module's own tensors and runs where they are."""
        if audio_emb.dim() != 3 or video_emb.dim() != 3 or audio_emb.shape[0] != video_emb.shape[0] or audio_emb.shape[2] != video_emb.shape[2]:
            raise ValueError(f"pair_scores: audio_emb must be (G, P, D) and video_emb (G, Q, D), got {tuple(audio_emb.shape)} and "
                             f"{tuple(video_emb.shape)}")
        if audio_emb.numel() == 0 or video_emb.numel() == 0:
            raise ValueError("pair_scores: empty embeddings")
        head = self.pack(audio_emb.device).head if be is _Hip else fold_head(self.head)
        return run_pair_head(head, audio_emb.float().contiguous(), video_emb.float().contiguous(), be)

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, video: torch.Tensor) -> torch.Tensor:
        """audio (b, 1, 128, 204), video (b, 3, f, h, w) already preprocessed -> scores (b,) f32"""
        if audio.shape[0] != video.shape[0]:
            raise ValueError(f"audio and video batch sizes differ: {audio.shape[0]} and {video.shape[0]}")
        return self.score_embeddings(self.embed_audio(audio), self.embed_video(video))


def load_avsync_model(model_path: str = DEFAULT_MODEL_PATH) -> AVSyncClassifier:
    """avsync_classifier.py:36-51: the three sub-folders of a trained classifier"""
    net = AVSyncClassifier(AudioConv2DNet.from_pretrained(os.path.join(model_path, "audio_encoder"), use_safetensors=False),
                           VideoR2Plus1DNet.from_pretrained(os.path.join(model_path, "video_encoder"), use_safetensors=False),
                           FCHead.from_pretrained(os.path.join(model_path, "head"), use_safetensors=False))
    net.eval()
    net.requires_grad_(False)
    return net


# ---- preprocessing: antialiased bicubic resize to 224 x 224 + CLIP normalisation ------------------------------------------------
def _cubic_aa(x):
    """Keys' cubic with a = -0.5 (the antialiasing resampler's kernel), evaluated in float32"""
    f = np.float32
    a, x = f(-0.5), np.abs(x)
    if x < f(1.0):
        return ((a + f(2.0)) * x - (a + f(3.0))) * x * x + f(1.0)
    if x < f(2.0):
        return (((x - f(5.0)) * x + f(8.0)) * x - f(4.0)) * a
    return f(0.0)


def resize_tables(in_size: int, out_size: int):
    """Taps of one axis of F.interpolate(mode="bicubic", antialias=True, align_corners=False): (start int32 [out], count int32 [out],
    weight f32 [out, taps]).  Output pixel i is centred at scale * (i + 0.5) and the kernel is stretched by the scale when shrinking,
    so that it low-passes; weights are normalised to sum 1 and zero past `count`.  Every step is rounded to float32 as torch's CPU
    implementation rounds it: near the far edge of a 256-pixel axis one float32 ulp of the centre moves a weight by 1e-5."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    support = f(2.0) * scale if scale >= f(1.0) else f(2.0)
    inv = f(1.0) / scale if scale >= f(1.0) else f(1.0)
    taps = int(np.ceil(support)) * 2 + 1
    start = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    weight = np.zeros((out_size, taps), np.float32)
    for i in range(out_size):
        center = scale * (f(i) + f(0.5))
        lo = max(int(center - support + f(0.5)), 0)
        n = min(int(center + support + f(0.5)), in_size) - lo
        total = f(0.0)
        for j in range(n):
            weight[i, j] = _cubic_aa((f(j + lo) - center + f(0.5)) * inv)
            total += weight[i, j]
        weight[i, :n] /= total
        start[i], count[i] = lo, n
    taps = min(taps, in_size)
    assert int(count.max()) <= taps
    return start, count, np.ascontiguousarray(weight[:, :taps])


class _ResizeTables:
    """taps for one (H, W), uploaded once per device"""

    def __init__(self):
        self._cache = {}

    def get(self, device, h: int, w: int, size: int):
        key = (str(device), h, w, size)
        t = self._cache.get(key)
        if t is None:
            t = tuple(tuple(torch.from_numpy(a).to(device) for a in resize_tables(n, size)) for n in (h, w))
            self._cache[key] = t
        return t


_RESIZE = _ResizeTables()


def preprocess_videos(videos: torch.Tensor, size: int = INPUT_SIZE, crop: int = INPUT_SIZE) -> torch.Tensor:
    """compute_avsync.py:14-34: (b, 3, t, h, w) in [0, 1] -> (b, 3, t, 224, 224) resized (bicubic, antialiased), centre-cropped and
    normalised with the CLIP constants.  The result is a (b, c, t, h, w) VIEW of channels-last memory, which the classifier reads
    without a copy."""
    if videos.dim() != 5 or videos.shape[1] != 3:
        raise ValueError(f"videos must be (b, 3, t, h, w), got {tuple(videos.shape)}")
    if crop != size:
        raise ValueError(f"centre crop {crop} of a {size} x {size} resize: only the reference's no-op crop is implemented")
    b, c, t, h, w = videos.shape
    frames = videos.float().permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w).contiguous()
    ytab, xtab = _RESIZE.get(frames.device, h, w, size)
    out = ops.resize_aa_normalize_f32(frames, ytab, xtab, size, crop, CLIP_MEAN, CLIP_STD)          # [b*t, size, size, 3]
    return out.view(b, t, size, size, 3).permute(0, 4, 1, 2, 3)


# ---- metrics -----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def compute_avsync_scores(audios: torch.Tensor, videos: torch.Tensor, net: AVSyncClassifier) -> torch.Tensor:
    """raw classifier scores (b,); videos (b, 3, t, h, w) in [0, 1]"""
    return net(audios, preprocess_videos(videos))


def relsync_from_scores(ref_scores: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """softmax([ref, own])[1] (compute_avsync.py:65-66)"""
    return torch.softmax(torch.stack([ref_scores, scores], dim=1), dim=1)[:, 1].contiguous()


@torch.no_grad()
def compute_relsync(audios: torch.Tensor, videos: torch.Tensor, net: AVSyncClassifier, ref_audios: Optional[torch.Tensor] = None,
                    ref_videos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """compute_avsync.py:49-68: exactly one of ref_audios / ref_videos; returns (b,) on the CPU like the reference"""
    if (ref_audios is None) == (ref_videos is None):
        raise ValueError("Please specify either ref_audios or ref_videos")
    v = net.embed_video(preprocess_videos(videos))
    a = net.embed_audio(audios)
    scores = net.score_embeddings(a, v)
    if ref_audios is not None:
        ref_scores = net.score_embeddings(net.embed_audio(ref_audios), v)
    else:
        ref_scores = net.score_embeddings(a, net.embed_video(preprocess_videos(ref_videos)))
    return relsync_from_scores(ref_scores, scores).detach().cpu()


_NETS: Dict[str, AVSyncClassifier] = {}


@torch.no_grad()
def compute_sync_metrics_on_av(audio_waveform: torch.Tensor, audio_sr: int, video: torch.Tensor,
                               ref_audio_waveform: Optional[torch.Tensor] = None, ref_audio_sr: Optional[int] = None,
                               ref_video: Optional[torch.Tensor] = None, metric: str = "alignsync", device=torch.device("cuda"),
                               dtype: torch.dtype = torch.float32, net: Optional[AVSyncClassifier] = None, clip_net=None):
    """compute_avsync.py:105-end: waveform (c, samples) at 16 kHz - or, under data_utils.set_resampler("device"), at any rate,
    resampled on the device as compute_avsync.py:141,157 do with torchaudio - video (3, 12, h, w) in [0, 1].  `net` defaults to
    load_avsync_model() (loaded once per process).  metric="alignsync" needs `ref_video` and `clip_net`, the ImageBind towers of
    asva_amd.imagebind_eval.load_clip_model(path): their checkpoint is not fetched here."""
    from .audio_features import resample, waveform_to_melspectrogram
    from .data_utils import get_resampler

    if metric not in ("alignsync", "relsync", "avsync_score"):
        raise ValueError(f"unknown metric {metric!r}")
    if metric == "alignsync" and clip_net is None:
        raise NotImplementedError("alignsync multiplies RelSync by an ImageBind image-audio similarity and no ImageBind checkpoint is "
                                  "fetched here: pass clip_net=load_clip_model(path) (asva_amd.imagebind_eval)")
    if dtype != torch.float32:
        raise ValueError("the scorer computes in float32 only")
    if video.dim() != 4 or video.shape[1] != 12:
        raise ValueError("video should be (3, 12, h, w): 12 frames at 6 FPS")
    if metric == "alignsync" and (ref_video is None or tuple(ref_video.shape) != tuple(video.shape)):
        raise ValueError("To compute alignsync, ref_video is needed as reference, and in the same shape as video")
    if metric == "relsync" and (ref_audio_waveform is None) == (ref_video is None):
        raise ValueError("To compute relsync, either ref_audio_waveform or ref_video is needed as reference")
    ref_audio_sr = audio_sr if ref_audio_sr is None else ref_audio_sr
    for sr in (audio_sr,) + ((ref_audio_sr,) if ref_audio_waveform is not None else ()):
        if sr != 16000 and get_resampler() != "device":
            raise ValueError(f"audio at {sr} Hz: resample to 16000 Hz first, or let this function do it on the device with "
                             'asva_amd.data_utils.set_resampler("device") / AVSD_RESAMPLER=device')
    if audio_sr != 16000:
        audio_waveform = resample(audio_waveform, audio_sr, 16000, device=device)
    if ref_audio_waveform is not None and ref_audio_sr != 16000:
        ref_audio_waveform = resample(ref_audio_waveform, ref_audio_sr, 16000, device=device)
    if net is None:
        net = _NETS.get(str(device))
        if net is None:
            net = _NETS[str(device)] = load_avsync_model().to(device)

    def mel(wave):
        return waveform_to_melspectrogram(wave, device=device).unsqueeze(0).contiguous()      # (1, 1, n_mel, t)

    audio = mel(audio_waveform)
    video = video.unsqueeze(0).to(device=device, dtype=dtype)
    if metric == "avsync_score":
        return compute_avsync_scores(audio, video, net)[0]
    if metric == "alignsync":
        from .imagebind_eval import compute_alignsync

        return compute_alignsync(audio, video, ref_video.unsqueeze(0).to(device=device, dtype=dtype), net, clip_net.to(device))[0]
    if ref_audio_waveform is not None:
        return compute_relsync(audio, video, net, ref_audios=mel(ref_audio_waveform))[0]
    return compute_relsync(audio, video, net, ref_videos=ref_video.unsqueeze(0).to(device=device, dtype=dtype))[0]


# ---- the classifier's own objective and evaluation: the head on a matrix of pairs --------------------------------------------------
def _embed_pairs(net: AVSyncClassifier, audios: torch.Tensor, videos: torch.Tensor, be):
    """audios (b, k, 1, n, t), videos (b, k, 3, f, h, w) -> embeddings (b, k, D) each: all b k clips in one pass per network"""
    if audios.dim() != 5 or videos.dim() != 6 or tuple(audios.shape[:2]) != tuple(videos.shape[:2]):
        raise ValueError(f"audios must be (b, k, 1, n, t) and videos (b, k, 3, f, h, w) with the same b and k, got {tuple(audios.shape)} and "
                         f"{tuple(videos.shape)}")
    b, k = audios.shape[:2]
    a, v = net._audio_cl(audios.flatten(0, 1)), net._video_cl(videos.flatten(0, 1))
    if be is _Hip:
        pk = net.pack(audios.device)
        fa, fv = pk.audio, pk.video
    else:
        fa, fv = fold_audio(net.audio_encoder), fold_video(net.video_encoder)
    return run_audio(fa, a, be).view(b, k, -1), run_video(fv, v, be).view(b, k, -1)


class AVSyncContrastiveTrainer(nn.Module):
    """avsync/models/sync_contrastive_trainer.py:9-60: the classifier's contrastive objective.  `forward` runs the head on all k x k
    (audio p, video q) pairs of each example and returns (av_loss, va_loss, av_acc, va_acc): the cross-entropy of every audio over
    the k videos and of every video over the k audios, both with the aligned pair as the label and logits divided by `tau`, and the
    two top-1 accuracies.

    VALUES ONLY: the launches carry no autograd graph, so the four results are 0-d f32 device tensors without gradient.  This is the
    forward value of the objective (validation, monitoring, checking a checkpoint), not a training step."""

    def __init__(self, audio_encoder: AudioConv2DNet, video_encoder: VideoR2Plus1DNet, head: FCHead, tau: float = 1.0):
        super().__init__()
        self.audio_encoder = audio_encoder
        self.video_encoder = video_encoder
        self.head = head
        self.tau = tau
        self._net = [AVSyncClassifier(audio_encoder, video_encoder, head)]      # shares the modules; kept out of state_dict()

    @torch.no_grad()
    def forward(self, audios: torch.Tensor, videos: torch.Tensor, be=_Hip):
        """audios (b, k, 1, n, t), videos (b, k, 3, f, h, w), preprocessed -> (av_loss, va_loss, av_acc, va_acc)"""
        net = self._net[0]
        a, v = _embed_pairs(net, audios, videos, be)
        r = be.pair_xent(net.pair_scores(a, v, be), float(self.tau))
        return r["av_loss"], r["va_loss"], r["av_acc"], r["va_acc"]

    def save_pretrained(self, save_dir: str):
        for name in ("audio_encoder", "video_encoder", "head"):
            getattr(self, name).save_pretrained(os.path.join(save_dir, name))


@torch.no_grad()
def shift_accuracy(net: AVSyncClassifier, audios: torch.Tensor, videos: torch.Tensor, tolerate_range: int = 5, be=_Hip) -> Dict[str, torch.Tensor]:
    """scripts/avsync_eval.py:116-148 for one batch: audios (b, k, 1, n, t) and videos (b, k, 3, f, h, w) are k clips per example, shifted
    by a fixed step.  All b k clips are embedded once; the centre audio (index k // 2) is scored against the k videos (one
    `pair_scores` call with P = 1) and the k audios against the centre video (one with Q = 1).  -> av_pred, va_pred (b,) int64: the
    argmax over videos / audios (a tie goes to the lowest index), av_hit, va_hit (b,) bool: |pred - centre| <= tolerate_range."""
    a, v = _embed_pairs(net, audios, videos, be)
    c = a.shape[1] // 2
    av = be.pair_xent(net.pair_scores(a[:, c:c + 1], v, be), 1.0)["row_argmax"][:, 0].long()
    va = be.pair_xent(net.pair_scores(a, v[:, c:c + 1], be), 1.0)["col_argmax"][:, 0].long()
    return {"av_pred": av, "va_pred": va, "av_hit": (av - c).abs() <= int(tolerate_range), "va_hit": (va - c).abs() <= int(tolerate_range)}


def evaluate_shift_accuracy(net: AVSyncClassifier, batches, tolerate_range: int = 5, be=_Hip) -> Dict[str, float]:
    """scripts/avsync_eval.py:111-167: `batches` yields dicts with "index" (b,) integers, "audio" (b, k, 1, n, t) and "video"
    (b, k, 3, f, h, w).  An example index seen more than once (a loader that replaced an unreadable file, several processes) counts
    once and its FIRST occurrence wins.  -> {"av_acc", "va_acc", "valid_examples"}"""
    seen: Dict[int, tuple] = {}
    for batch in batches:
        r = shift_accuracy(net, batch["audio"], batch["video"], tolerate_range, be)
        for i, a, v in zip(torch.as_tensor(batch["index"]).reshape(-1).tolist(), r["av_hit"].tolist(), r["va_hit"].tolist()):
            seen.setdefault(int(i), (float(a), float(v)))
    if not seen:
        raise ValueError("evaluate_shift_accuracy: no examples")
    n = len(seen)
    return {"av_acc": sum(a for a, _ in seen.values()) / n, "va_acc": sum(v for _, v in seen.values()) / n, "valid_examples": n}


# ---- shifted clips of one recording (avsync/data.py:21-75, 206-248), float64 on the host ---------------------------------------------
SAMPLING_TYPES = ("random-compact", "center-compact", "random", "uniform")
END_POINT_NUDGE = 1e-4        # seconds: a clip's first frame time moves in and its end moves back by this much


def uniform_starts(start: float, end: float, num: int, endpoint: bool = True) -> np.ndarray:
    """`num` equally spaced values over [start, end]: the first and last ON the end points, or (endpoint=False) every value at the
    centre of one of `num` equal cells, i.e. both ends pulled in by half a cell"""
    lo, hi = float(start), float(end)
    if not endpoint:
        half_cell = (hi - lo) / (2 * num)
        lo, hi = lo + half_cell, hi - half_cell
    if num == 1:
        return np.array([lo], dtype=np.float64)
    return lo + (hi - lo) * (np.arange(num, dtype=np.float64) / (num - 1))


def clip_starts(start: float, end: float, num: int, gap: float, sampling: str = "center-compact", rng=None) -> np.ndarray:
    """start times (float64 [num]) of `num` clips in [start, end]: "center-compact" / "random-compact" `gap` apart, centred or at a
    random offset; "random" at least `gap` apart, drawn one after the other; "uniform" spread from `start` to `end` whatever `gap`.
    `rng`: a random.Random for the two random types (a fresh one when None).  A range shorter than (num - 1) * gap is refused."""
    if sampling not in SAMPLING_TYPES:
        raise ValueError(f"sampling must be one of {SAMPLING_TYPES}, got {sampling!r}")
    start, end, gap = float(start), float(end), float(gap)
    if sampling == "uniform":
        return uniform_starts(start, end, num, endpoint=True)
    span = (num - 1) * gap                         # from the first start to the last
    slack = (end - start) - span                   # what is left of the range to place the first start in
    if slack < 0:
        raise ValueError(f"a range of {end - start:g} s ({start:g} .. {end:g}) cannot hold {num} clip starts {gap:g} s apart")
    if rng is None:
        rng = random.Random()
    steps = gap * np.arange(num, dtype=np.float64)
    if sampling == "center-compact":
        return (start + slack / 2.0) + steps
    if sampling == "random-compact":
        return rng.uniform(start, start + slack) + steps
    # "random": clip i is drawn between the earliest time its predecessor allows and the latest that leaves room for the rest
    starts = np.empty(num, dtype=np.float64)
    earliest = start
    for i in range(num):
        starts[i] = rng.uniform(earliest, end - (num - 1 - i) * gap)
        earliest = starts[i] + gap
    return starts


def clip_frame_seconds(starts: np.ndarray, video_num_frames: int = 12, video_fps: float = 6) -> np.ndarray:
    """(k, f + 1) float64: the f frame times of every clip and, last, its end; the first is moved 1e-4 s in and the end 1e-4 s back,
    so that rounding at the end points cannot pick a neighbour (data.py:239-243)"""
    offsets = np.arange(video_num_frames + 1, dtype=np.float64) / video_fps
    offsets[0] += END_POINT_NUDGE
    offsets[-1] -= END_POINT_NUDGE
    return np.asarray(starts, dtype=np.float64).reshape(-1, 1) + offsets


def nearest_frames(times: np.ndarray, frame_seconds: np.ndarray) -> np.ndarray:
    """index of the frame whose timestamp is nearest to each time; exactly between two frames the earlier one (argmin's first)"""
    return np.abs(np.asarray(times, dtype=np.float64)[..., None] - np.asarray(frame_seconds, dtype=np.float64)).argmin(axis=-1)


@torch.no_grad()
def shifted_pairs(frames: torch.Tensor, frame_seconds, waveform: torch.Tensor, sample_rate: int, *, num_clips: int = 31,
                  shift_time: float = 0.04, video_fps: float = 6, video_num_frames: int = 12, sampling: str = "center-compact", rng=None,
                  device=None, counts: Optional[dict] = None):
    """One recording -> the `num_clips` shifted (audio, video) clips of AudioVideoAlignedMultiPairDataset.__getitem__
    (avsync/data.py:206-248): frames (F, 3, H, W) in [0, 1] with timestamps frame_seconds [F], waveform (c, S) at sample_rate ->
    (audios (k, 1, 128, 204), videos (k, 3, f, 224, 224)) on the device, ready for `shift_accuracy` / AVSyncContrastiveTrainer.
    A host-side index list plus existing device calls: every DISTINCT frame the clips use is resized and normalised once
    (`preprocess_videos`' kernel) and then gathered; each clip's audio is the sample range [round(t0 sr), round(t1 sr)) of the
    waveform, resampled to 16 kHz on the device when needed, then `waveform_to_melspectrogram`.  `counts`, if a dict, receives
    "frames_resized".

    KNOWN DIVERGENCE: the reference gathers whole container audio packets whose timestamp falls in the clip, which cannot be
    reproduced without its decoder; the cut here is sample-exact instead.  The per-clip random horizontal flip (`randflip`, a training
    augmentation the evaluation switches off) is not built."""
    from .audio_features import resample, waveform_to_melspectrogram

    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames must be (F, 3, H, W), got {tuple(frames.shape)}")
    fs = np.asarray(frame_seconds, dtype=np.float64).reshape(-1)
    if fs.shape[0] != frames.shape[0]:
        raise ValueError(f"{frames.shape[0]} frames but {fs.shape[0]} timestamps")
    if fs.shape[0] == 0:
        raise ValueError("frames is empty")
    if waveform.dim() != 2 or waveform.shape[1] == 0:
        raise ValueError(f"waveform must be (channels, samples), got {tuple(waveform.shape)}")
    sample_rate = int(sample_rate)
    device = torch.device("cuda" if device is None else device)
    clip_duration = video_num_frames / video_fps
    duration = min(float(fs[-1]) + (float(fs[1] - fs[0]) if len(fs) > 1 else 0.0), waveform.shape[1] / sample_rate)
    if duration < clip_duration + (num_clips - 1) * shift_time:
        raise ValueError(f"a recording of {duration:.3f} s is too short for {num_clips} clips of {clip_duration:.3f} s shifted by {shift_time} s")
    times = clip_frame_seconds(clip_starts(0.0, duration - clip_duration, num_clips, shift_time, sampling, rng), video_num_frames, video_fps)
    # video: resize the distinct frames once, gather the clips from them
    idx = nearest_frames(times[:, :-1], fs)                                          # (k, f)
    used, inverse = np.unique(idx.reshape(-1), return_inverse=True)
    if counts is not None:
        counts["frames_resized"] = int(used.shape[0])
    src = frames[torch.from_numpy(used)].to(device=device, dtype=torch.float32)       # (U, 3, H, W)
    pre = preprocess_videos(src.permute(1, 0, 2, 3)[None])[0]                         # (3, U, 224, 224), a view of channels-last memory
    videos = pre[:, torch.from_numpy(inverse).to(device)].view(3, num_clips, video_num_frames, INPUT_SIZE, INPUT_SIZE).permute(1, 0, 2, 3, 4)
    # audio: the sample-exact range of every clip
    audios = []
    for t0, t1 in zip(times[:, 0], times[:, -1]):
        cut = waveform[:, int(round(t0 * sample_rate)):int(round(t1 * sample_rate))].to(device=device, dtype=torch.float32)
        if sample_rate != 16000:
            cut = resample(cut.contiguous(), sample_rate, 16000, device=device)
        audios.append(waveform_to_melspectrogram(cut, device=device))
    return torch.stack(audios), videos


def shifted_pairs_from_avi(filename: str, **kw):
    """`shifted_pairs` on one of the project's own .avi files (Motion-JPEG + PCM, asva_amd/video_io.py): frame i is stamped i / fps"""
    from .video_io import read_mjpeg_avi

    video, fps, audio, audio_fps = read_mjpeg_avi(filename)
    if audio is None:
        raise ValueError(f"{filename}: no audio stream")
    frames = video.permute(0, 3, 1, 2).float() / 255.0
    return shifted_pairs(frames, np.arange(frames.shape[0], dtype=np.float64) / fps, audio, audio_fps, **kw)
