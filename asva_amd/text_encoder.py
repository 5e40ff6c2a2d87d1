"""CLIP text encoder and tokenizer of Stable Diffusion 1.5, on the device.

`CLIPTextModel` mirrors the `text_encoder` the reference loads through transformers
(avgen/pipelines/pipeline_audio_cond_animation.py:83-119, :498): token + position embedding, pre-LN blocks with causal
self-attention and a quick-GELU MLP, a final LayerNorm.  The class is a parameter holder with SD1.5's `state_dict()` layout; the
arithmetic runs in libavsd_hip.so (csrc/clip_text.hip, and csrc/avsync.hip for the linear layers).  Everything is f32 on the
f32-input matrix cores, in the bf16 and the fp16 build of the library alike: the reference stores and feeds fp32 text encodings,
and a conditioning tensor must not move with the storage mode (bf16, fp16, split, plan) of the clip it conditions.

`CLIPTokenizer` is a pure-Python restatement of the byte-level BPE tokenizer of CLIP (vocab.json + merges.txt).

No real SD1.5 checkpoint or vocabulary was available when this was written: both classes are pinned against transformers with
seeded weights and a synthetic vocabulary (tests/golden/clip_text/), and agreement with the reference's published class-encoding
files has not been measured.
"""
from __future__ import annotations

import json
import os
import unicodedata
from typing import Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import ops
from .weights import _Pk, pack_device

CONFIG_NAME = "config.json"
WEIGHT_NAMES = ("model.safetensors", "pytorch_model.bin", "diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")
# CLIPTextConfig defaults of transformers (SD1.5's text_encoder/config.json overrides them: 768 / 3072 / 12 / 12, quick_gelu)
DEFAULT_CONFIG = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                      num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                      attention_dropout=0.0, pad_token_id=1, bos_token_id=49406, eos_token_id=49407)
HEAD_DIM = 64


class _Config(dict):
    """config.json as a dict with attribute access (`model.config.eos_token_id`, as transformers' config objects read)"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class TextModelOutput:
    """`[0]` / `.last_hidden_state` (b, L, C) and `[1]` / `.pooler_output` (b, C), as transformers' BaseModelOutputWithPooling"""

    def __init__(self, last_hidden_state: torch.Tensor, pooler_output: torch.Tensor):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = pooler_output

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]

    def __iter__(self):
        return iter((self.last_hidden_state, self.pooler_output))


# ---- parameter holders: module names are SD1.5's state-dict names ----------------------------------------------------------------
class _Attention(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(c, c) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, c: int, inter: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, inter), nn.Linear(inter, c)


class _Layer(nn.Module):
    def __init__(self, c: int, inter: int, eps: float):
        super().__init__()
        self.self_attn = _Attention(c)
        self.layer_norm1 = nn.LayerNorm(c, eps=eps)
        self.mlp = _MLP(c, inter)
        self.layer_norm2 = nn.LayerNorm(c, eps=eps)


class _Embeddings(nn.Module):
    def __init__(self, vocab: int, positions: int, c: int):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, c)
        self.position_embedding = nn.Embedding(positions, c)


class _Encoder(nn.Module):
    def __init__(self, n: int, c: int, inter: int, eps: float):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(c, inter, eps) for _ in range(n)])


class _TextTransformer(nn.Module):
    def __init__(self, cfg: Dict):
        super().__init__()
        c = cfg["hidden_size"]
        self.embeddings = _Embeddings(cfg["vocab_size"], cfg["max_position_embeddings"], c)
        self.encoder = _Encoder(cfg["num_hidden_layers"], c, cfg["intermediate_size"], cfg["layer_norm_eps"])
        self.final_layer_norm = nn.LayerNorm(c, eps=cfg["layer_norm_eps"])


def _f32_blob(tensors: List[torch.Tensor], device) -> List[torch.Tensor]:
    """the tensors as views of ONE f32 device buffer (256-byte-aligned items): the unit a launch plan ships as a CONST region"""
    offs, total = [], 0
    for t in tensors:
        offs.append(total)
        total += (t.numel() + 63) // 64 * 64
    blob = torch.zeros(total, dtype=torch.float32, device=device)
    views = []
    for t, o in zip(tensors, offs):
        v = blob[o:o + t.numel()].view(t.shape)
        v.copy_(t.detach().to(torch.float32))
        views.append(v)
    return [blob] + views


class CLIPTextModel(nn.Module):
    """transformers.CLIPTextModel for SD1.5's text_encoder: `model(input_ids)[0]` is the (b, 77, 768) f32 conditioning"""

    PREFIX = "text_model."

    def __init__(self, config: Optional[Dict] = None, **kw):
        super().__init__()
        cfg = dict(DEFAULT_CONFIG)
        cfg.update({k: v for k, v in dict(config or {}, **kw).items() if not k.startswith("_")})
        self._check_config(cfg)
        for k in ("architectures", "model_type"):          # what save_pretrained stamps the file with, not a setting
            cfg.pop(k, None)
        self._config = cfg
        self.text_model = _TextTransformer(cfg)
        self._packed: Dict[str, _Pk] = {}
        self.requires_grad_(False)
        self.eval()

    @staticmethod
    def _check_config(cfg: Dict) -> None:
        if cfg["hidden_act"] != "quick_gelu":
            raise NotImplementedError(f"hidden_act={cfg['hidden_act']!r}: only CLIP's quick_gelu is implemented (SD2's text encoder uses gelu)")
        c, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        if heads < 1 or c % heads or c // heads != HEAD_DIM:
            raise NotImplementedError(f"hidden_size {c} with {heads} heads: the attention kernel is built for a head dim of {HEAD_DIM}")
        if cfg["max_position_embeddings"] > 128:
            raise NotImplementedError("max_position_embeddings above 128: the attention kernel is built for sequences of up to 128 tokens")
        if "WithProjection" in "".join(cfg.get("architectures") or []):
            raise NotImplementedError("CLIPTextModelWithProjection: the projection head is not implemented")

    # ---- surface ----------------------------------------------------------------------------------------------------------------
    @property
    def config(self) -> _Config:
        return _Config(self._config)

    @property
    def device(self) -> torch.device:
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    def to(self, *args, **kw):
        """moves to a device; a dtype is accepted and ignored — the encoder computes and returns f32 whatever the pipeline's I/O dtype"""
        device = kw.get("device")
        for a in args:
            if isinstance(a, (str, torch.device, int)):
                device = a
        if device is not None:
            super().to(device)
        return self

    def half(self):
        return self

    def float(self):
        return self

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._packed = {}
        return r

    @classmethod
    def from_config(cls, config: Dict, **kw) -> "CLIPTextModel":
        return cls(config, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, subfolder: Optional[str] = "text_encoder", **_) -> "CLIPTextModel":
        path = os.path.join(pretrained_model_path, subfolder) if subfolder else pretrained_model_path
        with open(os.path.join(path, CONFIG_NAME)) as f:
            model = cls(json.load(f))
        for name in WEIGHT_NAMES:
            file = os.path.join(path, name)
            if os.path.isfile(file):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file

                    sd = load_file(file)
                else:
                    sd = torch.load(file, map_location="cpu", weights_only=True)
                model.load_state_dict(sd)
                return model
        raise FileNotFoundError(f"none of {', '.join(WEIGHT_NAMES)} under {path}")

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True) -> None:
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, CONFIG_NAME), "w") as f:
            json.dump({"architectures": ["CLIPTextModel"], "model_type": "clip_text_model", **self._config}, f, indent=2)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        if safe_serialization:
            from safetensors.torch import save_file

            save_file(sd, os.path.join(save_directory, WEIGHT_NAMES[0]))
        else:
            torch.save(sd, os.path.join(save_directory, WEIGHT_NAMES[1]))

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """SD1.5's names, with or without the `text_model.` prefix; `embeddings.position_ids` is ignored; a missing or an unknown
        tensor raises KeyError naming it"""
        own = super().state_dict()
        sd = {}
        for k, v in state_dict.items():
            k = k if k.startswith(self.PREFIX) else self.PREFIX + k
            if k.endswith("embeddings.position_ids"):
                continue
            if k not in own:
                raise KeyError(f"CLIPTextModel.load_state_dict: unexpected tensor {k!r}")
            sd[k] = v.to(torch.float32)
        for k in own:
            if k not in sd:
                raise KeyError(f"CLIPTextModel.load_state_dict: missing tensor {k!r}")
        r = super().load_state_dict(sd, strict=True)
        self._packed = {}
        return r

    # ---- packing ------------------------------------------------------------------------------------------------------------------
    def pack(self, device=None) -> _Pk:
        """state_dict -> f32 tables and kernel-layout weights (q|k|v fused to one [3C][C] matrix) inside one device buffer; cached per
        device, repacked after load_state_dict / .to().  Not keyed by precision.pack_key(): nothing here depends on the storage mode."""
        device = pack_device(device)
        if device is None and len(self._packed) == 1 and str(self.device) in self._packed:
            return self._packed[str(self.device)]
        device = pack_device(device, self.device, ops, "CLIPTextModel.pack")
        pk = self._packed.get(str(device))
        if pk is not None:
            return pk
        tm = self.text_model
        flat: List[torch.Tensor] = [tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight,
                                    tm.final_layer_norm.weight, tm.final_layer_norm.bias]
        for ly in tm.encoder.layers:
            a = ly.self_attn
            flat += [ly.layer_norm1.weight, ly.layer_norm1.bias,
                     torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]), torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]),
                     a.out_proj.weight, a.out_proj.bias, ly.layer_norm2.weight, ly.layer_norm2.bias,
                     ly.mlp.fc1.weight, ly.mlp.fc1.bias, ly.mlp.fc2.weight, ly.mlp.fc2.bias]
        views = _f32_blob(flat, device)
        names = ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")
        layers = [_Pk(**dict(zip(names, views[5 + 12 * i:17 + 12 * i]))) for i in range(len(tm.encoder.layers))]
        pk = _Pk(blob=views[0], tok=views[1], pos=views[2], lnf_g=views[3], lnf_b=views[4], layers=layers)
        self._packed[str(device)] = pk
        return pk

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def eos_positions(self, input_ids: torch.Tensor) -> torch.Tensor:
        """row of the pooled output: argmax(input_ids) under SD1.5's legacy eos_token_id == 2, else the first position equal to
        eos_token_id (position 0 when there is none), as transformers does"""
        ids = input_ids.to(torch.int)
        if self._config["eos_token_id"] == 2:
            return ids.argmax(dim=-1)
        return (ids == self._config["eos_token_id"]).int().argmax(dim=-1)

    _linear = staticmethod(ops.linear_f32)

    def encode_ids(self, ids: torch.Tensor, b: int, seq: int, pk: Optional[_Pk] = None) -> torch.Tensor:
        """the launches alone: ids int32 [b * seq] on the device, already checked -> [b * seq, C] after final_layer_norm"""
        pk = self.pack(ids.device) if pk is None else pk
        heads, eps = self._config["num_attention_heads"], self._config["layer_norm_eps"]
        c = self._config["hidden_size"]
        x = ops.embed_tokens_f32(ids, pk.tok, pk.pos, b, seq)
        for ly in pk.layers:
            qkv = self._linear(ops.layernorm_f32(x, ly.ln1_g, ly.ln1_b, eps), ly.wqkv, ly.bqkv)
            a = ops.attention_causal_f32(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], b, seq, heads)
            x = self._linear(a, ly.wo, ly.bo, res=x)
            h = self._linear(ops.layernorm_f32(x, ly.ln2_g, ly.ln2_b, eps), ly.w1, ly.b1)
            x = self._linear(ops.quick_gelu_f32(h, out=h), ly.w2, ly.b2, res=x)
        return ops.layernorm_f32(x, pk.lnf_g, pk.lnf_b, eps)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids=None,
                output_hidden_states: Optional[bool] = None, output_attentions: Optional[bool] = None, return_dict: Optional[bool] = None,
                **kw) -> TextModelOutput:
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise NotImplementedError("a padding mask (zeros in attention_mask) is not implemented; SD1.5 encodes without one")
        if output_hidden_states or output_attentions:
            raise NotImplementedError("output_hidden_states / output_attentions are not implemented")
        if position_ids is not None:
            raise NotImplementedError("explicit position_ids are not implemented")
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
        if input_ids.dim() != 2 or input_ids.is_floating_point():
            raise ValueError(f"input_ids must be integer (b, L), got {tuple(input_ids.shape)} {input_ids.dtype}")
        b, seq = input_ids.shape
        if seq > self._config["max_position_embeddings"]:
            raise NotImplementedError(f"sequence length {seq} exceeds max_position_embeddings {self._config['max_position_embeddings']}")
        host = input_ids.detach().cpu()
        # the entry point cannot see device data: the range is checked here
        if seq < 1 or int(host.min()) < 0 or int(host.max()) >= self._config["vocab_size"]:
            raise ValueError(f"input_ids must lie in [0, {self._config['vocab_size']}) and the sequence must not be empty")
        dev = self.device
        ids = host.to(torch.int32).contiguous().view(-1).to(dev)
        out = self.encode_ids(ids, b, seq).view(b, seq, -1)
        pooled = out[torch.arange(b, device=dev), self.eos_positions(host).to(dev)]
        return TextModelOutput(out, pooled)


# ---- tokenizer -----------------------------------------------------------------------------------------------------------------------
BOS, EOS = "<|startoftext|>", "<|endoftext|>"
_SPECIAL = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|"
# the split pattern for `regex`, and the same classes in `re` terms for when `regex` cannot be imported: letters = word characters that
# are neither digits nor "_".  (`re` knows the decimal digits Nd only; the other numerals of \p{N}, such as superscripts, then split as
# letters do.)
_SPLIT_REGEX = _SPECIAL + r"[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
_SPLIT_RE = _SPECIAL + r"[^\W\d_]+|\d|(?:[^\s\w]|_)+"


def _compile_split():
    """(split pattern, whitespace pattern), on `regex` when it can be imported and on `re` otherwise"""
    try:
        import regex
    except ImportError:
        import re

        return re.compile(_SPLIT_RE), re.compile(r"\s+")
    return regex.compile(_SPLIT_REGEX), regex.compile(r"\s+")


_SPLIT, _SPACE = _compile_split()


def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's byte alphabet: printable latin-1 bytes stand for themselves, the other 68 map to U+0100 onwards"""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    table, n = {}, 0
    for byte in range(256):
        if byte in keep:
            table[byte] = chr(byte)
        else:
            table[byte] = chr(256 + n)
            n += 1
    return table


class TokenizerOutput(dict):
    """`.input_ids` / `.attention_mask` (also as dict keys, so `model(**out)` works)"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class CLIPTokenizer:
    """transformers.CLIPTokenizer restated: NFC, whitespace runs to one space, lower-casing; CLIP's split pattern; byte-level BPE with
    the `</w>` end-of-word mark; `<|startoftext|>` first, `<|endoftext|>` last and as padding; truncation keeps the final EOS"""

    def __init__(self, vocab: Dict[str, int], merges: Sequence, model_max_length: int = 77, bos_token: str = BOS, eos_token: str = EOS,
                 pad_token: str = EOS, unk_token: str = EOS):
        self.encoder = dict(vocab)
        self.ranks = {tuple(m.split() if isinstance(m, str) else m): i for i, m in enumerate(merges)}
        self.model_max_length = int(model_max_length)
        self.bos_token, self.eos_token, self.pad_token, self.unk_token = bos_token, eos_token, pad_token, unk_token
        for t in (bos_token, eos_token, pad_token, unk_token):
            if t not in self.encoder:
                raise KeyError(f"CLIPTokenizer: the vocabulary lacks the special token {t!r}")
        self.bos_token_id, self.eos_token_id = self.encoder[bos_token], self.encoder[eos_token]
        self.pad_token_id, self.unk_token_id = self.encoder[pad_token], self.encoder[unk_token]
        self._bytes = bytes_to_unicode()
        self._cache: Dict[str, List[int]] = {}

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, subfolder: Optional[str] = "tokenizer", **_) -> "CLIPTokenizer":
        path = os.path.join(pretrained_model_path, subfolder) if subfolder else pretrained_model_path
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            lines = f.read().split("\n")
        merges = [ln for ln in lines if ln and not ln.startswith("#version")]
        kw = {}
        cfg_path = os.path.join(path, "tokenizer_config.json")
        if os.path.isfile(cfg_path):
            with open(cfg_path, encoding="utf-8") as f:
                cfg = json.load(f)
            if isinstance(cfg.get("model_max_length"), int) and 0 < cfg["model_max_length"] < 1 << 20:
                kw["model_max_length"] = cfg["model_max_length"]
            for key in ("bos_token", "eos_token", "pad_token", "unk_token"):
                tok = cfg.get(key)
                tok = tok.get("content") if isinstance(tok, dict) else tok
                if isinstance(tok, str):
                    kw[key] = tok
        return cls(vocab, merges, **kw)

    def __len__(self):
        return len(self.encoder)

    def _bpe(self, word: str) -> List[int]:
        """one pre-token (already in the byte alphabet) -> ids: the lowest-ranked adjacent pair merges first, leftmost first"""
        ids = self._cache.get(word)
        if ids is not None:
            return ids
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        while len(sym) > 1:
            best, at = None, -1
            for i in range(len(sym) - 1):
                r = self.ranks.get((sym[i], sym[i + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, i
            if best is None:
                break
            a, b2 = sym[at], sym[at + 1]
            out, i = [], 0
            while i < len(sym):
                if i + 1 < len(sym) and sym[i] == a and sym[i + 1] == b2:
                    out.append(a + b2)
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
        ids = [self.encoder.get(s, self.unk_token_id) for s in sym]
        self._cache[word] = ids
        return ids

    def tokenize_ids(self, text: str) -> List[int]:
        """ids of the text alone, without BOS / EOS"""
        text = _SPACE.sub(" ", unicodedata.normalize("NFC", text)).lower()
        ids: List[int] = []
        for piece in _SPLIT.findall(text):
            if piece in (self.bos_token, self.eos_token):
                ids.append(self.encoder[piece])
            else:
                ids += self._bpe("".join(self._bytes[b] for b in piece.encode("utf-8")))
        return ids

    def __call__(self, texts: Union[str, Sequence[str]], padding: Union[bool, str] = False, max_length: Optional[int] = None,
                 truncation: bool = False, return_tensors: Optional[str] = None, **_) -> TokenizerOutput:
        single = isinstance(texts, str)
        max_length = self.model_max_length if max_length is None else int(max_length)
        rows = []
        for t in ([texts] if single else list(texts)):
            ids = [self.bos_token_id] + self.tokenize_ids(t) + [self.eos_token_id]
            if truncation and len(ids) > max_length:
                ids = ids[:max_length - 1] + [self.eos_token_id]
            rows.append(ids)
        if padding == "max_length":
            width = max_length
        elif padding in (True, "longest"):
            width = max(len(r) for r in rows)
        else:
            width = None
        masks = [[1] * len(r) for r in rows]
        if width is not None:
            masks = [m + [0] * (width - len(m)) for m in masks]
            rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            if len({len(r) for r in rows}) > 1:
                raise ValueError("return_tensors='pt' needs rows of one length: pass padding=")
            ids_out = torch.tensor(rows, dtype=torch.long).view(len(rows), -1)
            mask_out = torch.tensor(masks, dtype=torch.long).view(len(rows), -1)
        elif return_tensors is None:
            ids_out, mask_out = (rows[0], masks[0]) if single else (rows, masks)
        else:
            raise ValueError(f"return_tensors={return_tensors!r}: only 'pt' or None")
        return TokenizerOutput(input_ids=ids_out, attention_mask=mask_out)
