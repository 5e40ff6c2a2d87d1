"""AVSync scorer: the reference's audio-video synchronisation classifier and the RelSync metric on it, on the device.

Mirrors avsync/models/{audio,video,head,avsync_classifier}.py (an R(2+1)D-18 video network, a 2-D convolutional audio network
on the log-mel spectrogram, a 3-layer FC head) and avgen/evaluations/avsync/compute_avsync.py (preprocessing, raw score, RelSync).
The classes below are parameter holders with the reference's constructor arguments and `state_dict()` layout; the arithmetic
runs in libavsd_hip.so (csrc/avsync.hip): every convolution, with its eval-mode BatchNorm folded into weights, bias and residual
scale at pack time, is one `avsd_convnd_f32` launch.

Everything is f32 on the f32-input matrix cores, in the bf16 and the fp16 build of the library alike: a score must not move with
the storage mode of the clip it judges.  No host synchronisation inside `forward`; all launches go to the current stream.

No trained classifier checkpoint was available when this was written: the path is pinned against the reference's modules with
seeded weights (tests/golden/avsync_tiny.pt), and no RelSync value of a real clip has been measured.
"""
from __future__ import annotations

import os
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
