"""CLIPSim and AlignSync on the device: the ImageBind-Huge vision, text and audio towers the reference's evaluation embeds with.

`CLIPModel` mirrors avgen/evaluations/models/clip.py:23-80 (`encode_image`, `encode_audio`, `encode_text`, `forward` ->
{"ia_sim", "it_sim"}); `compute_clip_consistency` and `compute_alignsync` mirror avgen/evaluations/clip/compute_clip.py and
avgen/evaluations/avsync/compute_avsync.py:71-102.  The class is a parameter holder whose `state_dict()` has the key names of
ImageBind's own checkpoint (table `KEYS`); the arithmetic runs in libavsd_hip.so:

  vision  ViT-H/14: patch embedding (avsd_convnd_f32, taps (1, 14, 14), stride 14, on the channels-last output of the preprocessing),
          cls + learned positions (avsd_vit_tokens_f32), pre-transformer LayerNorm, 32 pre-LN blocks of width 1280 (16 heads of 80,
          avsd_attention_f32; erf-GELU MLP 5120, avsd_gelu_f32), head = LayerNorm of the cls row + bias-free linear 1280 -> 1024.
          ImageBind's stem is a bias-free Conv3d with kernel (2, 14, 14) on the image repeated twice in time: at pack time it is
          folded to the sum of its two temporal slices, formed in f32.
  text    OpenCLIP-H: token + position embedding, 24 causal pre-LN blocks of width 1024 (16 heads of 64,
          avsd_attention_causal_f32), head = LayerNorm of the row at the first position holding the largest token id (ImageBind's
          argmax) + bias-free linear 1024 -> 1024.
  audio   the trunk of asva_amd/audio_encoder.py restated in f32: stem (taps (1, 16, 16), stride 10) + LayerNorm, 12 blocks of width
          768 (12 heads of 64) whose `bias_kv` pair is a 230th key written into the spare row of the fused q|k|v buffer, head
          LayerNorm + linear 768 -> 1024.  The 16-bit trunk is NOT used: a metric is f32 in both builds of the library and
          bit-identical between them, so that it does not move with the storage mode of the clip it judges.

All three `encode_*` return UNIT-NORM embeddings.  The reference multiplies the audio and text embeddings by the postprocessor's logit
scale and divides by it again (clip.py:41-45, 53-56); that round trip is skipped here, and the similarities are cosines computed by
avsd_cosine_rows_f32 with the norms of F.normalize.

No ImageBind checkpoint and none of ImageBind's sources were available when this was written.  The towers are pinned to
transformers' CLIPVisionModelWithProjection / CLIPTextModelWithProjection with seeded weights (tests/test_clipsim_cpu.py), the audio
trunk to a restatement of torch.nn.MultiheadAttention(add_bias_kv=True); the checkpoint key names in `KEYS` and the claim that
SD1.5's `tokenizer/` folder carries the BPE vocabulary of ImageBind are recalled, UNVERIFIED, and no IA, IT or AlignSync value of
a real clip has been measured.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import f32net, ops
from .weights import _Pk

DEFAULT_CHECKPOINT = ".checkpoints/imagebind_huge.pth"
EPS = 1e-6                  # every LayerNorm of the three trunks and heads
STEM_EPS = 1e-5             # the audio stem's norm_layer (nn.LayerNorm default)
TOWERS = ("vision", "text", "audio")
DEFAULT_CONFIG: Dict[str, Dict[str, int]] = {
    "vision": dict(image=224, patch=14, width=1280, heads=16, layers=32, mlp=5120, out=1024),
    "text": dict(vocab=49408, positions=77, width=1024, heads=16, layers=24, mlp=4096, out=1024),
    "audio": dict(mel=128, frames=204, patch=16, stride=10, width=768, heads=12, layers=12, mlp=3072, out=1024),
}

# ---- the ONE mapping table: short name -> key of ImageBind's checkpoint (`{}` = block index).  Recalled, unverified. ------------------
_BLOCK = {"n1_g": "norm_1.weight", "n1_b": "norm_1.bias", "in_w": "attn.in_proj_weight", "in_b": "attn.in_proj_bias",
          "out_w": "attn.out_proj.weight", "out_b": "attn.out_proj.bias", "n2_g": "norm_2.weight", "n2_b": "norm_2.bias",
          "fc1_w": "mlp.fc1.weight", "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias"}
KEYS: Dict[str, Dict[str, object]] = {
    "vision": {
        "cls": "modality_preprocessors.vision.cls_token",
        "stem_w": "modality_preprocessors.vision.rgbt_stem.proj.1.weight",
        "pos": "modality_preprocessors.vision.pos_embedding_helper.pos_embed",
        "pre_g": "modality_trunks.vision.pre_transformer_layer.0.weight",
        "pre_b": "modality_trunks.vision.pre_transformer_layer.0.bias",
        "block": ("modality_trunks.vision.blocks.{}.", _BLOCK),
        "head_g": "modality_heads.vision.0.weight", "head_b": "modality_heads.vision.0.bias", "head_w": "modality_heads.vision.2.weight",
    },
    "text": {
        "tok": "modality_preprocessors.text.token_embedding.weight",
        "pos": "modality_preprocessors.text.pos_embed",
        "block": ("modality_trunks.text.blocks.{}.", _BLOCK),
        "head_g": "modality_heads.text.proj.0.weight", "head_b": "modality_heads.text.proj.0.bias",
        "head_w": "modality_heads.text.proj.1.weight",
    },
    "audio": {      # the keys ImageBindSegmaskAudioEncoder.load_imagebind_checkpoint reads
        "cls": "modality_preprocessors.audio.cls_token",
        "stem_w": "modality_preprocessors.audio.rgbt_stem.proj.weight",
        "stem_g": "modality_preprocessors.audio.rgbt_stem.norm_layer.weight",
        "stem_b": "modality_preprocessors.audio.rgbt_stem.norm_layer.bias",
        "pos": "modality_preprocessors.audio.pos_embedding_helper.pos_embed",
        "block": ("modality_trunks.audio.blocks.{}.", dict(_BLOCK, bias_k="attn.bias_k", bias_v="attn.bias_v")),
        "head_g": "modality_heads.audio.0.weight", "head_b": "modality_heads.audio.0.bias", "head_w": "modality_heads.audio.2.weight",
    },
}


def n_tokens(tower: str, cfg: Dict[str, int]) -> int:
    """tokens of one sequence (without the audio trunk's spare row)"""
    if tower == "vision":
        return 1 + (cfg["image"] // cfg["patch"]) ** 2
    if tower == "text":
        return cfg["positions"]
    return 1 + ((cfg["mel"] - cfg["patch"]) // cfg["stride"] + 1) * ((cfg["frames"] - cfg["patch"]) // cfg["stride"] + 1)


def tower_keys(tower: str, cfg: Dict[str, int]) -> Dict[str, Tuple[str, List[int]]]:
    """short name (`blocks.N.<name>` inside a block) -> (checkpoint key, shape) of one tower, in a fixed order"""
    c, mlp, out, n = cfg["width"], cfg["mlp"], cfg["out"], n_tokens(tower, cfg)
    shapes = {"cls": [1, 1, c], "pos": [1, n, c], "pre_g": [c], "pre_b": [c], "stem_g": [c], "stem_b": [c], "head_g": [c], "head_b": [c],
              "head_w": [out, c], "n1_g": [c], "n1_b": [c], "in_w": [3 * c, c], "in_b": [3 * c], "out_w": [c, c], "out_b": [c], "n2_g": [c],
              "n2_b": [c], "fc1_w": [mlp, c], "fc1_b": [mlp], "fc2_w": [c, mlp], "fc2_b": [c], "bias_k": [1, 1, c], "bias_v": [1, 1, c]}
    if tower == "vision":
        shapes["stem_w"] = [c, 3, 2, cfg["patch"], cfg["patch"]]
    elif tower == "audio":
        shapes["stem_w"] = [c, 1, cfg["patch"], cfg["patch"]]
    else:
        shapes["tok"] = [cfg["vocab"], c]
    table: Dict[str, Tuple[str, List[int]]] = {}
    for name, key in KEYS[tower].items():
        if name == "block":
            prefix, names = key
            for i in range(cfg["layers"]):
                for short, tail in names.items():
                    table[f"blocks.{i}.{short}"] = (prefix.format(i) + tail, shapes[short])
        else:
            table[name] = (key, shapes[name])
    return table


def state_dict_shapes(config: Dict[str, Dict[str, int]]) -> Dict[str, List[int]]:
    """checkpoint key -> shape for the towers `config` names"""
    return {key: shape for tower in TOWERS if tower in config for key, shape in tower_keys(tower, config[tower]).values()}


class CLIPModel(f32net.F32Net):
    """avgen/evaluations/models/clip.py:23-80 on the device library.  `config` maps tower name -> geometry (DEFAULT_CONFIG: ImageBind-Huge);
    a tower that `config` leaves out is not built, and its `encode_*` raises.  Parameters are created uninitialised: load a state dict."""

    def __init__(self, config: Optional[Dict[str, Dict[str, int]]] = None, tokenizer=None):
        super().__init__()
        config = DEFAULT_CONFIG if config is None else config
        self._config = {t: dict(config[t]) for t in TOWERS if t in config}
        for t, cfg in self._config.items():
            self._check(t, cfg)
            f32net.declare(self, dict(tower_keys(t, cfg).values()))
        self.tokenizer = tokenizer
        self.eval()

    @staticmethod
    def _check(tower: str, cfg: Dict[str, int]) -> None:
        d = cfg["width"] // cfg["heads"] if cfg["heads"] > 0 and cfg["width"] % cfg["heads"] == 0 else 0
        if d not in ((64,) if tower == "text" else (64, 80)):
            raise NotImplementedError(f"{tower} tower: width {cfg['width']} with {cfg['heads']} heads; the attention kernels are built for "
                                      f"head dims {'64' if tower == 'text' else '64 and 80'}")
        if tower == "text" and cfg["positions"] > 128:
            raise NotImplementedError("text tower: the causal attention kernel is built for sequences of up to 128 tokens")
        if tower == "vision" and cfg["image"] % cfg["patch"]:
            raise ValueError("vision tower: the image size must be a multiple of the patch size")
        if tower != "text" and cfg["patch"] > 16:
            raise NotImplementedError(f"{tower} tower: patches of more than 16 x 16 pixels")

    # ---- surface ----------------------------------------------------------------------------------------------------------------
    @property
    def config(self) -> Dict[str, Dict[str, int]]:
        return {t: dict(c) for t, c in self._config.items()}

    # ImageBind's checkpoint is the state dict of the whole multi-modal model: the tensors of other modalities are ignored, and any
    # subset will do that holds every tensor of the towers this model was built with (a missing one raises KeyError naming it)
    STRICT_KEYS = False

    # ---- packing ------------------------------------------------------------------------------------------------------------------
    def _fold(self, sd) -> _Pk:
        """kernel layouts: stem weights tap-major and channels-last, the vision stem folded over time, cls / pos / bias_kv flattened.
        Every item is f32, so the contents do not depend on the storage mode."""
        root = _Pk()
        for tower, cfg in self._config.items():
            c = cfg["width"]
            t = _Pk()
            for name, (key, _) in tower_keys(tower, cfg).items():
                w = sd[key].detach().to(torch.float32)
                if name == "stem_w":
                    if tower == "vision":
                        w = w[:, :, 0] + w[:, :, 1]                                  # the image repeated twice in time: one f32 sum
                    w = w.permute(0, 2, 3, 1).reshape(c, -1)                         # [cout, kh * kw * cin]: tap-major, cin-minor
                elif name in ("cls", "pos") or name.endswith(("bias_k", "bias_v")):
                    w = w.reshape(-1, c) if name == "pos" else w.reshape(c)
                holder, leaf = t, name
                if name.startswith("blocks."):
                    _, i, leaf = name.split(".")
                    if not hasattr(t, "blocks"):                                     # created where the table has the blocks: the
                        t.blocks = [_Pk() for _ in range(cfg["layers"])]             # blob's items follow the order of the table
                    holder = t.blocks[int(i)]
                setattr(holder, leaf, w)
            setattr(root, tower, t)
        return root

    def _after_pack(self, root: _Pk) -> None:
        for t in self._config:                                                       # bias_k | bias_v as one row of 2 C values
            for blk in getattr(root, t).blocks:
                if hasattr(blk, "bias_k"):
                    blk.bias_kv = torch.cat([blk.bias_k, blk.bias_v])

    def _tower(self, name: str, device) -> Tuple[Dict[str, int], _Pk]:
        if name not in self._config:
            raise RuntimeError(f"CLIPModel: the {name} tower is not built (the checkpoint held no modality_*.{name}.* tensors)")
        return self._config[name], getattr(self.pack(device), name)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _head(self, rows: torch.Tensor, t: _Pk) -> torch.Tensor:
        """rows [b, C] (any row stride) -> LayerNorm, bias-free linear, L2 normalisation: (b, out) unit-norm"""
        e = ops.linear_f32(ops.layernorm_f32(rows, t.head_g, t.head_b, EPS), t.head_w, None)
        return ops.normalize_rows_f32(e, out=e)

    @torch.no_grad()
    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """images (n, 3, S, S), already resized and CLIP-normalised (S = 224 for ImageBind-Huge) -> (n, 1024) unit-norm"""
        cfg, t = self._tower("vision", images.device)
        s, p = cfg["image"], cfg["patch"]
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, s, s):
            raise ValueError(f"images must be (n, 3, {s}, {s}), got {tuple(images.shape)}")
        n, seq = images.shape[0], n_tokens("vision", cfg)
        x = images.float().permute(0, 2, 3, 1).contiguous().view(n, 1, s, s, 3)     # no copy for the output of preprocess_videos
        emb = ops.convnd_f32(x, t.stem_w, (1, p, p), (1, p, p), (0, 0, 0)).view(n * (seq - 1), -1)
        h = ops.vit_tokens_f32(emb, t.cls, t.pos, n)
        h = ops.layernorm_f32(h, t.pre_g, t.pre_b, EPS, out=h)
        h = f32net.run_blocks(h, t.blocks, n, seq, cfg["heads"], EPS)
        return self._head(h.view(n, seq, -1)[:, 0], t)

    @torch.no_grad()
    def encode_audio(self, audios: torch.Tensor) -> torch.Tensor:
        """audios (n, 1, 128, 204) mel-spectrograms -> (n, 1024) unit-norm"""
        cfg, t = self._tower("audio", audios.device)
        if audios.dim() != 4 or tuple(audios.shape[1:]) != (1, cfg["mel"], cfg["frames"]):
            raise ValueError(f"audios must be (n, 1, {cfg['mel']}, {cfg['frames']}), got {tuple(audios.shape)}")
        n, seq, p, st = audios.shape[0], n_tokens("audio", cfg) + 1, cfg["patch"], cfg["stride"]      # + the bias_kv slot
        x = audios.float().contiguous().view(n, 1, cfg["mel"], cfg["frames"], 1)
        emb = ops.convnd_f32(x, t.stem_w, (1, p, p), (1, st, st), (0, 0, 0)).view(n * (seq - 2), -1)
        emb = ops.layernorm_f32(emb, t.stem_g, t.stem_b, STEM_EPS, out=emb)
        h = ops.vit_tokens_f32(emb, t.cls, t.pos, n, tail_rows=1)
        h = f32net.run_blocks(h, t.blocks, n, seq, cfg["heads"], EPS)
        return self._head(h.view(n, seq, -1)[:, 0], t)

    def tokenize(self, texts: Sequence[str]) -> torch.Tensor:
        if self.tokenizer is None:
            raise ValueError("CLIPModel.encode_text: strings need a tokenizer (load_clip_model(tokenizer=...)); without one pass "
                             "integer ids (n, 77)")
        cfg = self._config.get("text", DEFAULT_CONFIG["text"])
        return self.tokenizer(list(texts), padding="max_length", max_length=cfg["positions"], truncation=True, return_tensors="pt").input_ids

    @torch.no_grad()
    def encode_text(self, texts: Union[Sequence[str], torch.Tensor]) -> torch.Tensor:
        """strings (tokenised with the model's CLIPTokenizer) or integer ids (n, 77) -> (n, 1024) unit-norm"""
        if "text" not in self._config:
            self._tower("text", None)
        ids = texts if isinstance(texts, torch.Tensor) else self.tokenize([texts] if isinstance(texts, str) else texts)
        dev = self.device
        cfg, t = self._tower("text", dev)
        if ids.dim() != 2 or ids.is_floating_point() or ids.shape[1] != cfg["positions"]:
            raise ValueError(f"text ids must be integer (n, {cfg['positions']}), got {tuple(ids.shape)} {ids.dtype}")
        host = ids.detach().cpu()
        if int(host.min()) < 0 or int(host.max()) >= cfg["vocab"]:                  # the entry point cannot see device data
            raise ValueError(f"text ids must lie in [0, {cfg['vocab']})")
        n, seq = host.shape
        h = ops.embed_tokens_f32(host.to(torch.int32).contiguous().view(-1).to(dev), t.tok, t.pos, n, seq)
        h = f32net.run_blocks(h, t.blocks, n, seq, cfg["heads"], EPS, causal=True)
        rows = h.view(n, seq, -1)[torch.arange(n, device=dev), host.argmax(dim=-1).to(dev)]      # the first largest id: end of text
        return self._head(rows, t)

    @torch.no_grad()
    def similarities(self, images: torch.Tensor, audios: Optional[torch.Tensor] = None, texts=None, rep: int = 1) -> Dict[str, torch.Tensor]:
        """as `forward`, with ONE audio / text per `rep` consecutive images: each is embedded once and broadcast by the cosine kernel"""
        img = self.encode_image(images)
        out = {}
        if audios is not None:
            out["ia_sim"] = ops.cosine_rows_f32(img, self.encode_audio(audios), rep)
        if texts is not None:
            out["it_sim"] = ops.cosine_rows_f32(img, self.encode_text(texts), rep)
        return out

    def forward(self, images: torch.Tensor, audios: Optional[torch.Tensor] = None, texts=None) -> Dict[str, torch.Tensor]:
        """clip.py:59-74: images (n, 3, 224, 224), audios (n, 1, 128, 204), texts n strings or ids (n, 77) -> {"ia_sim": (n,), "it_sim": (n,)}"""
        return self.similarities(images, audios, texts, rep=1)


def load_clip_model(checkpoint: str = DEFAULT_CHECKPOINT, tokenizer=None, config: Optional[Dict[str, Dict[str, int]]] = None) -> CLIPModel:
    """clip.py:76-80.  `checkpoint`: ImageBind's own `imagebind_huge.pth` (or a state dict already loaded).  `tokenizer`: a CLIPTokenizer, or the
    folder of one (vocab.json + merges.txt).  A tower whose tensors are all absent from the checkpoint is left unbuilt; one that is
    partly there raises KeyError naming what is missing."""
    sd = checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu", weights_only=True)
    config = DEFAULT_CONFIG if config is None else config
    built = {}
    for tower in TOWERS:
        if tower in config and any(key in sd for key, _ in tower_keys(tower, config[tower]).values()):
            built[tower] = config[tower]
    if "vision" not in built:
        raise KeyError("load_clip_model: the checkpoint holds no modality_*.vision.* tensors; every similarity needs the vision tower")
    if isinstance(tokenizer, str):
        from .text_encoder import CLIPTokenizer

        tokenizer = CLIPTokenizer.from_pretrained(tokenizer, subfolder=None)
    model = CLIPModel(built, tokenizer=tokenizer)
    model.load_state_dict(sd)
    return model


# ---- metrics -----------------------------------------------------------------------------------------------------------------------
def preprocess_videos(videos: torch.Tensor, audios: Optional[torch.Tensor] = None, texts=None, size: int = 224):
    """compute_clip.py:8-38: videos (b, f, 3, H, W) in [0, 1] -> ((b f), 3, 224, 224) resized (bicubic, antialiased) and CLIP-normalised
    on the device (the preprocessing of avsync.preprocess_videos), audios and texts repeated per frame as the reference does"""
    from .avsync import preprocess_videos as _resize

    if videos.dim() != 5 or videos.shape[2] != 3:
        raise ValueError(f"videos must be (b, f, 3, h, w), got {tuple(videos.shape)}")
    b, f = videos.shape[:2]
    frames = _resize(videos.permute(0, 2, 1, 3, 4), size=size, crop=size)        # (b, 3, f, S, S), a view of channels-last memory
    frames = frames.permute(0, 2, 1, 3, 4).reshape(b * f, 3, size, size)         # (still a view: encode_image reads it without a copy)
    if audios is not None:
        audios = audios.repeat_interleave(f, dim=0).contiguous()
    if texts is not None:
        texts = texts.repeat_interleave(f, dim=0) if isinstance(texts, torch.Tensor) else [t for t in texts for _ in range(f)]
    return frames, audios, texts


@torch.no_grad()
def compute_clip_consistency(videos: torch.Tensor, audios: Optional[torch.Tensor] = None, texts=None, net: Optional[CLIPModel] = None):
    """compute_clip.py:41-54: videos (b, f, 3, H, W) in [0, 1], audios (b, 1, 128, 204), texts b strings or ids (b, 77) ->
    {"ia_sim": (b, f), "it_sim": (b, f)}.  Each clip's audio and text are embedded ONCE and broadcast over its f frames; the bits are
    those of net(images, audios, texts) on the reference's frame-repeated inputs."""
    if net is None:
        raise ValueError("compute_clip_consistency: pass net=load_clip_model(path)")
    b, f = videos.shape[:2]
    if audios is not None and audios.shape[0] != b or texts is not None and len(texts) != b:
        raise ValueError("compute_clip_consistency: one audio / text per clip")
    return {k: v.view(b, f) for k, v in net.similarities(preprocess_videos(videos, size=net.config["vision"]["image"])[0], audios, texts, rep=f).items()}


def alignsync_from_sims(ia_sims: torch.Tensor, relsync: torch.Tensor) -> torch.Tensor:
    """compute_avsync.py:93-100: ia_sims (b, f) of [ground-truth first frame, predicted frames 1..] -> mean over the predicted frames of
    softmax([first-frame sim, frame sim])[1], times RelSync"""
    first, pred = ia_sims[:, 0:1], ia_sims[:, 1:]
    probs = torch.softmax(torch.stack([first.expand_as(pred), pred], dim=2), dim=2)[:, :, 1].mean(dim=1)
    return probs * relsync


@torch.no_grad()
def compute_alignsync(audios: torch.Tensor, videos: torch.Tensor, ref_videos: torch.Tensor, net, clip_net: CLIPModel) -> torch.Tensor:
    """compute_avsync.py:71-102: videos, ref_videos (b, 3, f, H, W) in [0, 1], audios (b, 1, 128, 204) -> (b,) on the CPU"""
    from .avsync import compute_relsync

    if videos.dim() != 5 or videos.shape[2] < 2 or tuple(ref_videos.shape) != tuple(videos.shape):
        raise ValueError("compute_alignsync: videos and ref_videos must be (b, 3, f, h, w) of one shape with f >= 2")
    relsync = compute_relsync(audios, videos, net, ref_videos=ref_videos)
    mixed = torch.cat([ref_videos[:, :, 0:1], videos[:, :, 1:]], dim=2).permute(0, 2, 1, 3, 4)
    ia = compute_clip_consistency(mixed, audios, net=clip_net)["ia_sim"].detach().cpu()
    return alignsync_from_sims(ia, relsync)
