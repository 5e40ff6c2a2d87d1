"""fp32 functional restatement of the AVSync classifier in plain torch (F.conv3d, F.batch_norm, ...), taking a state dict.

It is the oracle of the device scorer (asva_amd/avsync.py) for shapes the fixture tests/golden/avsync_tiny.pt does not hold;
tests/test_avsync_cpu.py pins it to that fixture, which tools/gen_avsync_golden.py wrote from the reference's own modules
(avsync/models/{video,audio,head}.py).  Also here: the seeded weight recipe and the synthetic inputs the fixture was made with,
so that the tests re-draw the 83 MB of weights instead of storing them.
"""
import zlib

import torch
import torch.nn.functional as F

VIDEO_STAGES = (("conv2x", 1), ("conv3x", 2), ("conv4x", 2), ("conv5x", 2))
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _bn(x, sd, p, eps=1e-5):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, eps)


def video_forward(sd, x, stages=None):
    """sd: state dict of the video network; x (b, 3, f, h, w) preprocessed -> (b, 512).  `stages` receives the (b, c, f, h, w) output of
    conv1 (after its max-pool) and of the four stages."""
    x = F.relu(_bn(F.conv3d(x, sd["conv1.0.weight"], None, (1, 2, 2), (1, 3, 3)), sd, "conv1.1"))
    x = F.max_pool3d(x, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    if stages is not None:
        stages.append(x)
    for name, stride in VIDEO_STAGES:
        for i in range(2):
            p, s = f"{name}.{i}", stride if i == 0 else 1
            h = F.relu(_bn(F.conv3d(x, sd[p + ".spt_conv1.weight"], None, (1, s, s), (0, 1, 1)), sd, p + ".spt_bn1"))
            h = F.relu(_bn(F.conv3d(h, sd[p + ".tmp_conv1.weight"], None, (s, 1, 1), (1, 0, 0)), sd, p + ".tmp_bn1"))
            h = F.relu(_bn(F.conv3d(h, sd[p + ".spt_conv2.weight"], None, 1, (0, 1, 1)), sd, p + ".spt_bn2"))
            h = F.conv3d(h, sd[p + ".tmp_conv2.weight"], None, 1, (1, 0, 0))
            r = F.conv3d(x, sd[p + ".res_conv.weight"], None, (s, s, s)) if p + ".res_conv.weight" in sd else x
            x = F.relu(_bn(h + r, sd, p + ".out_bn"))
        if stages is not None:
            stages.append(x)
    return x.mean(dim=(2, 3, 4))


def audio_forward(sd, x, stages=None):
    """x (b, 1, n_mel, t) -> (b, 512); `stages` receives the output of conv1 and of the four blocks"""
    x = F.relu(_bn(F.conv2d(x, sd["conv1.0.weight"], None, 2, 3), sd, "conv1.1"))
    if stages is not None:
        stages.append(x)
    for i, s in ((1, 2), (2, 2), (3, 2), (4, 1)):
        p = f"block{i}"
        x = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"], None, s, 1), sd, p + ".bn1"))
        x = F.relu(_bn(F.conv2d(x, sd[p + ".conv2.weight"], None, 1, 1), sd, p + ".bn2"))
        if stages is not None:
            stages.append(x)
    return x.mean(dim=(2, 3))


def head_forward(sd, audio_emb, video_emb):
    y = torch.cat([audio_emb, video_emb], 1)
    y = F.relu(F.linear(y, sd["fc.0.weight"], sd["fc.0.bias"]))
    y = F.relu(F.linear(y, sd["fc.3.weight"], sd["fc.3.bias"]))
    return F.linear(y, sd["fc.6.weight"], sd["fc.6.bias"])


def classifier_forward(sd, audio, video):
    """sd: state dict of the whole classifier (audio_encoder. / video_encoder. / head.) -> scores (b,)"""
    a = audio_forward(_sub(sd, "audio_encoder."), audio)
    v = video_forward(_sub(sd, "video_encoder."), video)
    return head_forward(_sub(sd, "head."), a, v)[:, 0]


def relsync(ref_scores, scores):
    return torch.softmax(torch.stack([ref_scores, scores], 1), 1)[:, 1]


def preprocess(videos, size=224):
    """(b, 3, t, h, w) in [0, 1] -> (b, 3, t, size, size): what torchvision's Resize(antialias=True) + Normalize do for tensors"""
    b, c, t, h, w = videos.shape
    fr = videos.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    fr = F.interpolate(fr, size=(size, size), mode="bicubic", antialias=True, align_corners=False)
    fr = (fr - torch.tensor(CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    return fr.view(b, t, c, size, size).permute(0, 2, 1, 3, 4).contiguous()


# ---- seeded weights --------------------------------------------------------------------------------------------------------------
def draw_tensor(name, shape, seed):
    """One tensor of the recipe, from a CPU generator of its own seeded by (seed, crc32(name)): the draw does not depend on module order.
    Convolutions N(0, 2 / fan_in); BatchNorm weight U(0.5, 1), bias and running mean N(0, 0.1^2), running variance U(0.5, 1.5);
    linear weights N(0, 1 / in_features), biases N(0, 0.1^2).  Default initialisation cannot see a wrong kernel: with it the biases
    decide the score.  Neither can a smaller out_bn weight: with U(0.25, 0.6) the eight residual blocks shrink the signal to about 1 %
    of the accumulated biases, and the video embeddings of any two clips came out 1 - 4 % apart."""
    g = torch.Generator(device="cpu").manual_seed((int(seed) << 32) | zlib.crc32(name.encode()))
    leaf = name.rsplit(".", 1)[-1]
    shape = tuple(shape)
    if leaf == "num_batches_tracked":
        return torch.zeros(shape, dtype=torch.int64)
    if len(shape) >= 2:
        fan_in = 1
        for d in shape[1:]:
            fan_in *= d
        std = (1.0 / fan_in) ** 0.5 if len(shape) == 2 else (2.0 / fan_in) ** 0.5
        return torch.randn(shape, generator=g) * std
    if leaf == "running_var":
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == "weight":
        return 0.5 + 0.5 * torch.rand(shape, generator=g)
    return 0.1 * torch.randn(shape, generator=g)          # bias, running_mean


def draw_state_dict(shapes, seed):
    """shapes: {name: shape} (tests/golden/avsync_state_dict_shapes.json)"""
    return {k: draw_tensor(k, s, seed) for k, s in shapes.items()}


def check_draw(sd, probe):
    """probe: {name: (sum, first eight values)} stored with the fixture — catches a drift of torch's generator"""
    for k, (total, head) in probe.items():
        v = sd[k].double().reshape(-1)
        assert abs(v.sum().item() - total) <= 1e-9 * max(1.0, v.abs().sum().item()), f"{k}: the seeded draw changed (sum)"
        assert torch.equal(v[:len(head)], torch.as_tensor(head, dtype=torch.float64)), f"{k}: the seeded draw changed (first values)"


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------------
def grating_video_u8(frames, height, width, angle, speed, wavelength, phase=0.0, mean=0.5, contrast=0.45, colour=0.9):
    """(3, frames, height, width) uint8: a moving sinusoidal grating mean + contrast * sin(.), phase step `colour` per colour channel"""
    t = torch.arange(frames, dtype=torch.float64).view(1, frames, 1, 1)
    y = torch.arange(height, dtype=torch.float64).view(1, 1, height, 1)
    x = torch.arange(width, dtype=torch.float64).view(1, 1, 1, width)
    c = torch.arange(3, dtype=torch.float64).view(3, 1, 1, 1)
    a = torch.tensor(angle, dtype=torch.float64)
    arg = 2.0 * torch.pi * ((x * torch.cos(a) + y * torch.sin(a)) / wavelength - speed * t) + phase + colour * c
    return torch.round(255.0 * (mean + contrast * torch.sin(arg))).to(torch.uint8)


def u8_to_unit(u8):
    return u8.float() / 255.0


def normalize_clip(x):
    """(b, 3, ...) in [0, 1] -> CLIP-normalised (elementwise IEEE operations only: reproducible everywhere)"""
    shape = (1, 3) + (1,) * (x.dim() - 2)
    return (x - torch.tensor(CLIP_MEAN).view(shape)) / torch.tensor(CLIP_STD).view(shape)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
