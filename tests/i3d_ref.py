"""Plain-torch functional restatement of the Inception-v1 I3D (avgen/evaluations/models/pytorch_i3d.py:9-326 of the reference:
MaxPool3dSamePadding, Unit3D, InceptionModule, InceptionI3d), taking a state dict in that module's layout, and of the video
preprocessing of avgen/evaluations/fvd/compute_fvd.py.

Every window uses TensorFlow "same" padding computed from the input size (`same_pad`), applied with F.pad before an unpadded
F.conv3d / F.max_pool3d, as the reference does: a padded zero takes part in a maximum.  tools/gen_fvd_golden.py checks this file
against the reference module to <= 1e-12 rel-L2 in float64; it is the oracle of the device extractor (asva_amd/fvd.py) where the
reference does not exist.  Also here: the seeded weight recipe (the 12.7 M weights are re-drawn instead of stored) and the synthetic
clips of the fixture.
"""
import zlib

import torch
import torch.nn.functional as F

from tests.avsync_ref import rel_l2  # noqa: F401  (re-exported for the tests)

BN_EPS = 1e-5                # pytorch_i3d.py:71
NUM_CLASSES = 400
# (name, cin, [b0, b1a, b1b, b2a, b2b, b3b])
MIXED = [("Mixed_3b", 192, [64, 96, 128, 16, 32, 32]), ("Mixed_3c", 256, [128, 128, 192, 32, 96, 64]),
         ("Mixed_4b", 480, [192, 96, 208, 16, 48, 64]), ("Mixed_4c", 512, [160, 112, 224, 24, 64, 64]),
         ("Mixed_4d", 512, [128, 128, 256, 24, 64, 64]), ("Mixed_4e", 512, [112, 144, 288, 32, 64, 64]),
         ("Mixed_4f", 528, [256, 160, 320, 32, 128, 128]), ("Mixed_5b", 832, [256, 160, 320, 32, 128, 128]),
         ("Mixed_5c", 832, [384, 192, 384, 48, 128, 128])]
ENDPOINTS = ["Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b", "Mixed_3c",
             "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2", "Mixed_5b", "Mixed_5c"]
POOLS = {"MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)),
         "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)), "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2))}


def same_pad(size, k, s):
    """one axis -> (front, back): pytorch_i3d.py:73-95"""
    total = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return total // 2, total - total // 2


def pad_same(x, k, s):
    (tf, tb), (hf, hb), (wf, wb) = (same_pad(x.shape[2 + i], k[i], s[i]) for i in range(3))
    return F.pad(x, (wf, wb, hf, hb, tf, tb))


def _unit(sd, name, x, k, s=(1, 1, 1), eps=BN_EPS):
    """Unit3D: conv without bias on the same-padded input, BatchNorm in eval mode, ReLU"""
    x = F.conv3d(pad_same(x, k, s), sd[name + ".conv3d.weight"], None, s)
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                     False, 0.0, eps)
    return F.relu(x)


def _pool(x, k, s):
    return F.max_pool3d(pad_same(x, k, s), k, s)


def _mixed(sd, p, x, eps):
    b0 = _unit(sd, p + ".b0", x, (1, 1, 1), eps=eps)
    b1 = _unit(sd, p + ".b1b", _unit(sd, p + ".b1a", x, (1, 1, 1), eps=eps), (3, 3, 3), eps=eps)
    b2 = _unit(sd, p + ".b2b", _unit(sd, p + ".b2a", x, (1, 1, 1), eps=eps), (3, 3, 3), eps=eps)
    b3 = _unit(sd, p + ".b3b", _pool(x, (3, 3, 3), (1, 1, 1)), (1, 1, 1), eps=eps)
    return torch.cat([b0, b1, b2, b3], 1)


def forward(sd, x, stages=None, eps=BN_EPS):
    """x (b, 3, t, h, w) in (-1, 1) -> (b, 400): the logits averaged over the temporal positions the average pool leaves
    (InceptionI3d.forward); `stages`, if a dict, receives every endpoint's NCTHW output"""
    def mark(name, y):
        if stages is not None:
            stages[name] = y
        return y

    x = mark("Conv3d_1a_7x7", _unit(sd, "Conv3d_1a_7x7", x, (7, 7, 7), (2, 2, 2), eps))
    x = mark("MaxPool3d_2a_3x3", _pool(x, *POOLS["MaxPool3d_2a_3x3"]))
    x = mark("Conv3d_2b_1x1", _unit(sd, "Conv3d_2b_1x1", x, (1, 1, 1), eps=eps))
    x = mark("Conv3d_2c_3x3", _unit(sd, "Conv3d_2c_3x3", x, (3, 3, 3), eps=eps))
    x = mark("MaxPool3d_3a_3x3", _pool(x, *POOLS["MaxPool3d_3a_3x3"]))
    for name, _, _ in MIXED:
        if name == "Mixed_4b":
            x = mark("MaxPool3d_4a_3x3", _pool(x, *POOLS["MaxPool3d_4a_3x3"]))
        if name == "Mixed_5b":
            x = mark("MaxPool3d_5a_2x2", _pool(x, *POOLS["MaxPool3d_5a_2x2"]))
        x = mark(name, _mixed(sd, name, x, eps))
    x = F.avg_pool3d(x, (2, 7, 7), (1, 1, 1))
    x = F.conv3d(x, sd["logits.conv3d.weight"], sd["logits.conv3d.bias"])
    return x.squeeze(3).squeeze(3).mean(dim=2)


def preprocess(videos, sequence_length=None, size=224):
    """compute_fvd.py preprocess_videos for tensors: BCTHW in [0, 1] -> (B, 3, T, 224, 224) in (-1, 1)"""
    b, c, t, h, w = videos.shape
    if sequence_length is not None:
        assert sequence_length <= t
        videos = videos[:, :, :sequence_length]
        t = sequence_length
    frames = videos.permute(0, 2, 1, 3, 4).flatten(end_dim=1)
    frames = F.interpolate(frames, size=(size, size), mode="bicubic", antialias=True, align_corners=False)
    return frames.view(b, t, c, size, size).permute(0, 2, 1, 3, 4).contiguous() * 2 - 1


# ---- state-dict shapes (the reference module's layout), written to tests/golden/fvd/state_dict_shapes.json ------------------------------
def conv_shapes():
    s = {"Conv3d_1a_7x7": (64, 3, 7, 7, 7), "Conv3d_2b_1x1": (64, 64, 1, 1, 1), "Conv3d_2c_3x3": (192, 64, 3, 3, 3)}
    for n, cin, (o0, o1a, o1b, o2a, o2b, o3b) in MIXED:
        s.update({n + ".b0": (o0, cin, 1, 1, 1), n + ".b1a": (o1a, cin, 1, 1, 1), n + ".b1b": (o1b, o1a, 3, 3, 3),
                  n + ".b2a": (o2a, cin, 1, 1, 1), n + ".b2b": (o2b, o2a, 3, 3, 3), n + ".b3b": (o3b, cin, 1, 1, 1)})
    return s


def state_dict_shapes():
    shapes = {}
    for name, w in conv_shapes().items():
        shapes[name + ".conv3d.weight"] = list(w)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{leaf}"] = [w[0]]
        shapes[name + ".bn.num_batches_tracked"] = []
    shapes["logits.conv3d.weight"] = [NUM_CLASSES, 1024, 1, 1, 1]
    shapes["logits.conv3d.bias"] = [NUM_CLASSES]
    return shapes


# ---- seeded weights ---------------------------------------------------------------------------------------------------------------------
def draw_tensor(name, shape, seed):
    """One tensor of the recipe, from a CPU generator of its own seeded by (seed, crc32(name)).  The draw has to carry a signal through
    22 ReLU layers in series and four max pools: convolutions N(0, 2 / fan_in) (He: the second moment is carried through a ReLU),
    BatchNorm weight and running variance U(0.9, 1.1) (scale near 1), BatchNorm bias and running mean N(0, 0.1^2); the logits layer
    weight N(0, 1 / 1024), bias N(0, 0.1^2)."""
    g = torch.Generator(device="cpu").manual_seed((int(seed) << 32) | zlib.crc32(name.encode()))
    leaf = name.rsplit(".", 1)[-1]
    shape = tuple(shape)
    if leaf == "num_batches_tracked":
        return torch.zeros(shape, dtype=torch.int64)
    if len(shape) >= 2:
        fan_in = 1
        for d in shape[1:]:
            fan_in *= d
        std = (1.0 / fan_in) ** 0.5 if name.startswith("logits.") else (2.0 / fan_in) ** 0.5
        return torch.randn(shape, generator=g) * std
    if leaf == "running_var" or (leaf == "weight" and ".bn." in name):
        return 0.9 + 0.2 * torch.rand(shape, generator=g)
    return 0.1 * torch.randn(shape, generator=g)          # bias, running_mean


def draw_state_dict(shapes, seed):
    return {k: draw_tensor(k, s, seed) for k, s in shapes.items()}


def check_draw(sd, probe):
    """probe: {name: (sum, first eight values)} stored with the fixture — catches a drift of torch's generator"""
    for k, (total, head) in probe.items():
        v = sd[k].double().reshape(-1)
        assert abs(v.sum().item() - total) <= 1e-9 * max(1.0, v.abs().sum().item()), f"{k}: the seeded draw changed (sum)"
        assert torch.equal(v[:len(head)], torch.as_tensor(head, dtype=torch.float64)), f"{k}: the seeded draw changed (first values)"


# ---- synthetic clips --------------------------------------------------------------------------------------------------------------------
def clip_u8(frames, height, width, angle, wavelength, speed, mean=0.5, contrast=0.4, colour=0.9, seed=0):
    """(frames, 3, height, width) uint8: two crossed sinusoidal gratings that drift and turn from frame to frame, plus seeded pixel
    noise — structure in space and in time, so that the temporal windows have something to act on"""
    y = torch.arange(height, dtype=torch.float64).view(1, 1, height, 1)
    x = torch.arange(width, dtype=torch.float64).view(1, 1, 1, width)
    c = torch.arange(3, dtype=torch.float64).view(1, 3, 1, 1)
    f = torch.arange(frames, dtype=torch.float64).view(frames, 1, 1, 1)
    a = angle + 0.07 * f
    g1 = torch.sin(2.0 * torch.pi * (x * torch.cos(a) + y * torch.sin(a)) / wavelength + speed * f + colour * c)
    g2 = torch.sin(2.0 * torch.pi * (x * torch.sin(a) - y * torch.cos(a)) / (2.7 * wavelength) - 0.6 * speed * f + 1.3 * colour * c)
    noise = torch.rand((frames, 3, height, width), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    return torch.round(255.0 * (mean + contrast * (0.6 * g1 + 0.4 * g2) + 0.1 * noise)).clamp(0, 255).to(torch.uint8)


def u8_to_unit(u8):
    return u8.float() / 255.0


def clip_to_bcthw(u8):
    """(T, 3, H, W) uint8 -> (1, 3, T, H, W) float32 in [0, 1]"""
    return u8_to_unit(u8).permute(1, 0, 2, 3).unsqueeze(0).contiguous()
