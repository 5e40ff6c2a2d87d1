"""Plain-torch restatement of the three ImageBind towers asva_amd/imagebind_eval.py runs on the device (ViT vision tower with its
Conv3d stem on the twice-repeated image, causal text tower with the argmax pooling, audio trunk with MultiheadAttention's appended
bias_kv pair) and of the metric arithmetic, in fp32 or float64, parametrised by config, and the seeded weight recipe that
tools/gen_clipsim_golden.py and the tests share.  State dicts use the key names of ImageBind's checkpoint (the one mapping table,
asva_amd.imagebind_eval.KEYS).  tests/test_clipsim_cpu.py pins the vision and text towers to transformers."""
import math

import torch
import torch.nn.functional as F

from asva_amd.imagebind_eval import n_tokens, tower_keys

SEED = 20241018
QK_GAIN = 1.5          # q and k rows of in_proj ~ N(0, (QK_GAIN / sqrt(C))^2): a peaked softmax, so that a masking error moves the output
BIAS_KV_STD = 2.0      # the audio trunk's appended pair: large enough that dropping the 230th key misses every bound (gen_clipsim_golden.py)
EPS, STEM_EPS = 1e-6, 1e-5

# the small towers of the tests: v80 / v64 (56 x 56 image, 16 patches + cls, two heads of 80 / 64, 2 blocks), vh1 (ImageBind-Huge's
# geometry with ONE block), t64 (77 positions, two heads of 64, 2 blocks), a1 (the audio trunk's geometry with ONE block), and tiny
# audio / vision towers for the metric-level tests
CONFIGS = {
    "v80": {"vision": dict(image=56, patch=14, width=160, heads=2, layers=2, mlp=320, out=64)},
    "v64": {"vision": dict(image=56, patch=14, width=128, heads=2, layers=2, mlp=256, out=64)},
    "vh1": {"vision": dict(image=224, patch=14, width=1280, heads=16, layers=1, mlp=5120, out=1024)},
    "t64": {"text": dict(vocab=128, positions=77, width=128, heads=2, layers=2, mlp=256, out=64)},
    "a1": {"audio": dict(mel=128, frames=204, patch=16, stride=10, width=768, heads=12, layers=1, mlp=3072, out=1024)},
}
CONFIGS["tiny"] = {"vision": CONFIGS["v80"]["vision"], "text": CONFIGS["t64"]["text"],
                   "audio": dict(mel=128, frames=204, patch=16, stride=10, width=64, heads=1, layers=1, mlp=128, out=64)}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def draw_state_dict(config, seed=SEED):
    """the seeded weights of the towers `config` names: one generator, tensors drawn in the order of the mapping table"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for tower in ("vision", "text", "audio"):
        if tower not in config:
            continue
        c = config[tower]["width"]
        for name, (key, shape) in tower_keys(tower, config[tower]).items():
            t = torch.randn(shape, generator=g)
            leaf = name.split(".")[-1]
            if leaf.endswith("_g"):
                t = 1.0 + 0.1 * t
            elif leaf.endswith("_b"):
                t = 0.1 * t
            elif leaf in ("bias_k", "bias_v"):
                t = BIAS_KV_STD * t
            elif leaf in ("cls", "pos"):
                t = 0.5 * t
            elif leaf == "in_w":
                t[:2 * c] *= QK_GAIN / math.sqrt(c)
                t[2 * c:] /= math.sqrt(c)
            elif leaf == "stem_w":
                t = t / math.sqrt(t[0].numel())
            elif leaf != "tok":
                t = t / math.sqrt(shape[1])
            sd[key] = t.contiguous()
    return sd


def _named(sd, tower, cfg, dtype):
    return {name: sd[key].to(dtype) for name, (key, _) in tower_keys(tower, cfg).items()}


def _blocks(w, cfg, h, causal=False):
    """pre-LN blocks on h (b, L, C); with bias_k / bias_v one more key and value per sequence, as torch.nn.MultiheadAttention appends"""
    b, L, c = h.shape
    heads = cfg["heads"]
    d = c // heads
    for i in range(cfg["layers"]):
        p = f"blocks.{i}."
        qkv = F.linear(F.layer_norm(h, (c,), w[p + "n1_g"], w[p + "n1_b"], EPS), w[p + "in_w"], w[p + "in_b"])
        q, k, v = qkv.split(c, dim=-1)
        if p + "bias_k" in w:
            k = torch.cat([k, w[p + "bias_k"].expand(b, 1, c)], dim=1)
            v = torch.cat([v, w[p + "bias_v"].expand(b, 1, c)], dim=1)
        q, k, v = (t.view(b, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        logits = (q * d ** -0.5) @ k.transpose(-1, -2)
        if causal:
            logits = logits.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float("-inf"))
        a = (torch.softmax(logits, dim=-1) @ v).transpose(1, 2).reshape(b, L, c)
        h = h + F.linear(a, w[p + "out_w"], w[p + "out_b"])
        m = F.linear(F.layer_norm(h, (c,), w[p + "n2_g"], w[p + "n2_b"], EPS), w[p + "fc1_w"], w[p + "fc1_b"])
        h = h + F.linear(F.gelu(m), w[p + "fc2_w"], w[p + "fc2_b"])
    return h


def _head(w, rows):
    c = rows.shape[-1]
    return F.normalize(F.linear(F.layer_norm(rows, (c,), w["head_g"], w["head_b"], EPS), w["head_w"]), dim=-1)


def vision_stem(w, cfg, images):
    """ImageBind's stem as it stands: the image repeated twice in time through the bias-free Conv3d with kernel (2, p, p) -> (n, patches, C)"""
    p = cfg["patch"]
    x = F.conv3d(images[:, :, None].repeat(1, 1, 2, 1, 1), w["stem_w"], stride=(2, p, p))
    return x.flatten(2).transpose(1, 2)


def encode_image(sd, cfg, images, dtype=torch.float32, trunk_out=None):
    """images (n, 3, S, S) -> (n, out) unit-norm"""
    w = _named(sd, "vision", cfg, dtype)
    x = vision_stem(w, cfg, images.to(dtype))
    h = torch.cat([w["cls"].expand(x.shape[0], 1, -1), x], dim=1) + w["pos"]
    h = F.layer_norm(h, (h.shape[-1],), w["pre_g"], w["pre_b"], EPS)
    h = _blocks(w, cfg, h)
    if trunk_out is not None:
        trunk_out.append(h)
    return _head(w, h[:, 0])


def encode_text(sd, cfg, ids, dtype=torch.float32):
    """ids (n, 77) -> (n, out) unit-norm; the pooled row is the first position holding the largest id"""
    w = _named(sd, "text", cfg, dtype)
    h = _blocks(w, cfg, w["tok"][ids.long()] + w["pos"], causal=True)
    return _head(w, h[torch.arange(ids.shape[0]), ids.argmax(dim=-1)])


def encode_audio(sd, cfg, mels, dtype=torch.float32, bias_kv=True):
    """mels (n, 1, 128, 204) -> (n, out) unit-norm; bias_kv=False drops the appended pair (what a forgotten 230th key computes)"""
    w = _named(sd, "audio", cfg, dtype)
    if not bias_kv:
        w = {k: v for k, v in w.items() if not k.endswith(("bias_k", "bias_v"))}
    c = cfg["width"]
    x = F.conv2d(mels.to(dtype), w["stem_w"], stride=cfg["stride"]).flatten(2).transpose(1, 2)
    x = F.layer_norm(x, (c,), w["stem_g"], w["stem_b"], STEM_EPS)
    h = torch.cat([w["cls"].expand(x.shape[0], 1, -1), x], dim=1) + w["pos"]
    return _head(w, _blocks(w, cfg, h)[:, 0])


def cosine(x, y):
    return (F.normalize(x, dim=-1) * F.normalize(y, dim=-1)).sum(-1)


# ---- metrics (avgen/evaluations/clip/compute_clip.py, avgen/evaluations/avsync/compute_avsync.py:71-102) ------------------------------
def preprocess(videos, size):
    """videos (b, f, 3, H, W) in [0, 1] -> ((b f), 3, size, size): bicubic antialiased resize + CLIP normalisation, what torchvision's
    Resize / CenterCrop(no-op) / Normalize do"""
    b, f = videos.shape[:2]
    x = F.interpolate(videos.reshape(b * f, *videos.shape[2:]), size=(size, size), mode="bicubic", antialias=True, align_corners=False)
    mean = torch.tensor((0.48145466, 0.4578275, 0.40821073), dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711), dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def compute_clip_consistency(sd, config, videos, audios=None, ids=None, dtype=torch.float32):
    """the reference's way: every frame against its clip's audio / text, repeated per frame -> {"ia_sim": (b, f), "it_sim": (b, f)}"""
    b, f = videos.shape[:2]
    img = encode_image(sd, config["vision"], preprocess(videos.to(dtype), config["vision"]["image"]), dtype)
    out = {}
    if audios is not None:
        out["ia_sim"] = cosine(img, encode_audio(sd, config["audio"], audios.repeat_interleave(f, dim=0), dtype)).view(b, f)
    if ids is not None:
        out["it_sim"] = cosine(img, encode_text(sd, config["text"], ids.repeat_interleave(f, dim=0), dtype)).view(b, f)
    return out


def alignsync_from_sims(ia_sims, relsync):
    """ia_sims (b, f): column 0 the ground-truth first frame, columns 1.. the predicted frames"""
    first, pred = ia_sims[:, 0:1], ia_sims[:, 1:]
    probs = torch.softmax(torch.stack([first.expand_as(pred), pred], dim=2), dim=2)[:, :, 1].mean(dim=1)
    return probs * relsync


def compute_alignsync(sd, config, audios, videos, ref_videos, relsync, dtype=torch.float32):
    """videos, ref_videos (b, 3, f, H, W); `relsync` (b,) comes from the AVSync classifier"""
    mixed = torch.cat([ref_videos[:, :, 0:1], videos[:, :, 1:]], dim=2).permute(0, 2, 1, 3, 4)
    return alignsync_from_sims(compute_clip_consistency(sd, config, mixed, audios, dtype=dtype)["ia_sim"], relsync.to(dtype))


def make_ids(cfg, seed=SEED):
    """(4, 77) ids: end of text (the largest id, also the padding after it) early, in the last position only, at 30 with padding, at 1"""
    g = torch.Generator().manual_seed(seed + 1)
    L, top = cfg["positions"], cfg["vocab"] - 1
    ids = torch.randint(0, top - 1, (4, L), generator=g)
    ids[:, 0] = top - 1                                            # start of text
    for row, at in enumerate((5, L - 1, 30, 1)):
        ids[row, at:] = top
    return ids


def make_inputs(name, seed=SEED):
    """the seeded inputs of fixture `name` (tests/golden/clipsim/<name>.pt holds the outputs only: a 224 x 224 batch is over 1 MB)"""
    g = torch.Generator().manual_seed(seed + 2)
    config = CONFIGS[name]
    out = {}
    if "vision" in config and name != "tiny":
        s = config["vision"]["image"]
        out["images"] = torch.randn(2, 3, s, s, generator=g)
    if "audio" in config:
        out["audios"] = torch.randn(2, 1, config["audio"]["mel"], config["audio"]["frames"], generator=g)
    if "text" in config:
        out["ids"] = make_ids(config["text"])[:2] if name == "tiny" else make_ids(config["text"])
    if name == "tiny":
        out["videos"] = torch.rand(2, 3, 3, 40, 56, generator=g)                  # (b, f, 3, H, W)
    return out
