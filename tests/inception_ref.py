"""Plain-torch restatement of the pytorch-fid Inception-v3 (avgen/evaluations/models/inception_v3.py of the reference: torchvision's
Inception3(num_classes=1008, aux_logits=False) with the four patched block classes), taking a state dict in torchvision's layout.

Written by hand from the layer widths (torchvision is not installed where the fixtures are made): F.conv2d + F.batch_norm(eps 1e-3) +
ReLU for every BasicConv2d, and the three pooling calls exactly as the reference's block classes make them.  It is the oracle of the
device extractor (asva_amd/fid.py); tools/gen_fid_golden.py runs it in float64 for tests/golden/fid/fid_tiny.pt.  Also here: the
seeded weight recipe (the 24 M weights are re-drawn instead of stored) and the synthetic images of the fixture.
"""
import zlib

import torch
import torch.nn.functional as F

from tests.avsync_ref import rel_l2  # noqa: F401  (re-exported for the tests)

BN_EPS = 1e-3
NUM_CLASSES = 1008
STAGES = ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2", "Mixed_5b", "Mixed_5c",
          "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c"]


def _bc(sd, name, x, stride=1, padding=0):
    """BasicConv2d: conv without bias, BatchNorm(eps=1e-3) in eval mode, ReLU"""
    x = F.conv2d(x, sd[name + ".conv.weight"], None, stride, padding)
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                     False, 0.0, BN_EPS)
    return F.relu(x)


def _inception_a(sd, p, x):
    b1 = _bc(sd, p + ".branch1x1", x)
    b5 = _bc(sd, p + ".branch5x5_2", _bc(sd, p + ".branch5x5_1", x), padding=2)
    bd = _bc(sd, p + ".branch3x3dbl_1", x)
    bd = _bc(sd, p + ".branch3x3dbl_2", bd, padding=1)
    bd = _bc(sd, p + ".branch3x3dbl_3", bd, padding=1)
    bp = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)
    bp = _bc(sd, p + ".branch_pool", bp)
    return torch.cat([b1, b5, bd, bp], 1)


def _inception_b(sd, p, x):
    b3 = _bc(sd, p + ".branch3x3", x, stride=2)
    bd = _bc(sd, p + ".branch3x3dbl_1", x)
    bd = _bc(sd, p + ".branch3x3dbl_2", bd, padding=1)
    bd = _bc(sd, p + ".branch3x3dbl_3", bd, stride=2)
    bp = F.max_pool2d(x, kernel_size=3, stride=2)
    return torch.cat([b3, bd, bp], 1)


def _inception_c(sd, p, x):
    b1 = _bc(sd, p + ".branch1x1", x)
    b7 = _bc(sd, p + ".branch7x7_1", x)
    b7 = _bc(sd, p + ".branch7x7_2", b7, padding=(0, 3))
    b7 = _bc(sd, p + ".branch7x7_3", b7, padding=(3, 0))
    bd = _bc(sd, p + ".branch7x7dbl_1", x)
    bd = _bc(sd, p + ".branch7x7dbl_2", bd, padding=(3, 0))
    bd = _bc(sd, p + ".branch7x7dbl_3", bd, padding=(0, 3))
    bd = _bc(sd, p + ".branch7x7dbl_4", bd, padding=(3, 0))
    bd = _bc(sd, p + ".branch7x7dbl_5", bd, padding=(0, 3))
    bp = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)
    bp = _bc(sd, p + ".branch_pool", bp)
    return torch.cat([b1, b7, bd, bp], 1)


def _inception_d(sd, p, x):
    b3 = _bc(sd, p + ".branch3x3_1", x)
    b3 = _bc(sd, p + ".branch3x3_2", b3, stride=2)
    b7 = _bc(sd, p + ".branch7x7x3_1", x)
    b7 = _bc(sd, p + ".branch7x7x3_2", b7, padding=(0, 3))
    b7 = _bc(sd, p + ".branch7x7x3_3", b7, padding=(3, 0))
    b7 = _bc(sd, p + ".branch7x7x3_4", b7, stride=2)
    bp = F.max_pool2d(x, kernel_size=3, stride=2)
    return torch.cat([b3, b7, bp], 1)


def _inception_e(sd, p, x, max_pool):
    b1 = _bc(sd, p + ".branch1x1", x)
    b3 = _bc(sd, p + ".branch3x3_1", x)
    b3 = torch.cat([_bc(sd, p + ".branch3x3_2a", b3, padding=(0, 1)), _bc(sd, p + ".branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = _bc(sd, p + ".branch3x3dbl_1", x)
    bd = _bc(sd, p + ".branch3x3dbl_2", bd, padding=1)
    bd = torch.cat([_bc(sd, p + ".branch3x3dbl_3a", bd, padding=(0, 1)), _bc(sd, p + ".branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    if max_pool:     # Mixed_7c of the FID network (inception_v3.py:324)
        bp = F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
    else:
        bp = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)
    bp = _bc(sd, p + ".branch_pool", bp)
    return torch.cat([b1, b3, bd, bp], 1)


def forward(sd, x, stages=None):
    """x (b, 3, h, w) in (-1, 1) -> (features (b, 2048), logits (b, 1008)); `stages`, if a dict, receives every stage's NCHW output"""
    def mark(name, y):
        if stages is not None:
            stages[name] = y
        return y

    x = mark("Conv2d_1a_3x3", _bc(sd, "Conv2d_1a_3x3", x, stride=2))
    x = mark("Conv2d_2a_3x3", _bc(sd, "Conv2d_2a_3x3", x))
    x = mark("Conv2d_2b_3x3", _bc(sd, "Conv2d_2b_3x3", x, padding=1))
    x = mark("maxpool1", F.max_pool2d(x, kernel_size=3, stride=2))
    x = mark("Conv2d_3b_1x1", _bc(sd, "Conv2d_3b_1x1", x))
    x = mark("Conv2d_4a_3x3", _bc(sd, "Conv2d_4a_3x3", x))
    x = mark("maxpool2", F.max_pool2d(x, kernel_size=3, stride=2))
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = mark(n, _inception_a(sd, n, x))
    x = mark("Mixed_6a", _inception_b(sd, "Mixed_6a", x))
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = mark(n, _inception_c(sd, n, x))
    x = mark("Mixed_7a", _inception_d(sd, "Mixed_7a", x))
    x = mark("Mixed_7b", _inception_e(sd, "Mixed_7b", x, max_pool=False))
    x = mark("Mixed_7c", _inception_e(sd, "Mixed_7c", x, max_pool=True))
    feat = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    return feat, F.linear(feat, sd["fc.weight"], sd["fc.bias"])


def preprocess(images, size=229):
    """compute_fid.py:5-18 for tensors: BCHW in [0, 1] -> (B, 3, 229, 229) in (-1, 1)"""
    return F.interpolate(images, size=(size, size), mode="bicubic", antialias=True, align_corners=False) * 2 - 1


# ---- state-dict shapes (torchvision's layout), written to tests/golden/fid/state_dict_shapes.json by tools/gen_fid_golden.py ----------
def _a(n, cin, pf):
    return {n + ".branch1x1": (64, cin, 1, 1), n + ".branch5x5_1": (48, cin, 1, 1), n + ".branch5x5_2": (64, 48, 5, 5),
            n + ".branch3x3dbl_1": (64, cin, 1, 1), n + ".branch3x3dbl_2": (96, 64, 3, 3), n + ".branch3x3dbl_3": (96, 96, 3, 3),
            n + ".branch_pool": (pf, cin, 1, 1)}


def _c(n, cin, c7):
    return {n + ".branch1x1": (192, cin, 1, 1), n + ".branch7x7_1": (c7, cin, 1, 1), n + ".branch7x7_2": (c7, c7, 1, 7),
            n + ".branch7x7_3": (192, c7, 7, 1), n + ".branch7x7dbl_1": (c7, cin, 1, 1), n + ".branch7x7dbl_2": (c7, c7, 7, 1),
            n + ".branch7x7dbl_3": (c7, c7, 1, 7), n + ".branch7x7dbl_4": (c7, c7, 7, 1), n + ".branch7x7dbl_5": (192, c7, 1, 7),
            n + ".branch_pool": (192, cin, 1, 1)}


def _e(n, cin):
    return {n + ".branch1x1": (320, cin, 1, 1), n + ".branch3x3_1": (384, cin, 1, 1), n + ".branch3x3_2a": (384, 384, 1, 3),
            n + ".branch3x3_2b": (384, 384, 3, 1), n + ".branch3x3dbl_1": (448, cin, 1, 1), n + ".branch3x3dbl_2": (384, 448, 3, 3),
            n + ".branch3x3dbl_3a": (384, 384, 1, 3), n + ".branch3x3dbl_3b": (384, 384, 3, 1), n + ".branch_pool": (192, cin, 1, 1)}


def conv_shapes():
    s = {"Conv2d_1a_3x3": (32, 3, 3, 3), "Conv2d_2a_3x3": (32, 32, 3, 3), "Conv2d_2b_3x3": (64, 32, 3, 3), "Conv2d_3b_1x1": (80, 64, 1, 1),
         "Conv2d_4a_3x3": (192, 80, 3, 3)}
    s.update(_a("Mixed_5b", 192, 32))
    s.update(_a("Mixed_5c", 256, 64))
    s.update(_a("Mixed_5d", 288, 64))
    s.update({"Mixed_6a.branch3x3": (384, 288, 3, 3), "Mixed_6a.branch3x3dbl_1": (64, 288, 1, 1), "Mixed_6a.branch3x3dbl_2": (96, 64, 3, 3),
              "Mixed_6a.branch3x3dbl_3": (96, 96, 3, 3)})
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        s.update(_c(n, 768, c7))
    s.update({"Mixed_7a.branch3x3_1": (192, 768, 1, 1), "Mixed_7a.branch3x3_2": (320, 192, 3, 3), "Mixed_7a.branch7x7x3_1": (192, 768, 1, 1),
              "Mixed_7a.branch7x7x3_2": (192, 192, 1, 7), "Mixed_7a.branch7x7x3_3": (192, 192, 7, 1), "Mixed_7a.branch7x7x3_4": (192, 192, 3, 3)})
    s.update(_e("Mixed_7b", 1280))
    s.update(_e("Mixed_7c", 2048))
    return s


def state_dict_shapes():
    shapes = {}
    for name, w in conv_shapes().items():
        shapes[name + ".conv.weight"] = list(w)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{leaf}"] = [w[0]]
        shapes[name + ".bn.num_batches_tracked"] = []
    shapes["fc.weight"] = [NUM_CLASSES, 2048]
    shapes["fc.bias"] = [NUM_CLASSES]
    return shapes


# ---- seeded weights ---------------------------------------------------------------------------------------------------------------------
def draw_tensor(name, shape, seed):
    """One tensor of the recipe, from a CPU generator of its own seeded by (seed, crc32(name)).  The draw has to keep a ReLU network of
    about 47 layers in series alive: convolutions N(0, 2 / fan_in) (He: the second moment is carried through a ReLU), BatchNorm
    weight U(0.9, 1.1) and running variance U(0.9, 1.1) (scale near 1), BatchNorm bias and running mean N(0, 0.1^2) so that the
    biases neither vanish nor decide the features; fc weight N(0, 1 / 2048), fc bias N(0, 0.1^2)."""
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


# ---- synthetic images -------------------------------------------------------------------------------------------------------------------
def image_u8(height, width, angle, wavelength, phase=0.0, mean=0.5, contrast=0.4, colour=0.9, seed=0):
    """(3, height, width) uint8: two crossed sinusoidal gratings plus seeded pixel noise — structure at several scales, so that the
    antialiased resize and the deep layers both have something to act on"""
    y = torch.arange(height, dtype=torch.float64).view(1, height, 1)
    x = torch.arange(width, dtype=torch.float64).view(1, 1, width)
    c = torch.arange(3, dtype=torch.float64).view(3, 1, 1)
    a = torch.tensor(angle, dtype=torch.float64)
    g1 = torch.sin(2.0 * torch.pi * (x * torch.cos(a) + y * torch.sin(a)) / wavelength + phase + colour * c)
    g2 = torch.sin(2.0 * torch.pi * (x * torch.sin(a) - y * torch.cos(a)) / (2.7 * wavelength) + 1.3 * colour * c)
    noise = torch.rand((3, height, width), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    return torch.round(255.0 * (mean + contrast * (0.6 * g1 + 0.4 * g2) + 0.1 * noise)).clamp(0, 255).to(torch.uint8)


def u8_to_unit(u8):
    return u8.float() / 255.0
