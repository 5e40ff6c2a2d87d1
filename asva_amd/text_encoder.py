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

from . import f32net, modelio, ops
from .weights import _Pk

# transformers' names first (written as safetensors / torch.save), then diffusers'
WEIGHT_NAMES = ("model.safetensors", "pytorch_model.bin") + modelio.WEIGHT_NAMES
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


class CLIPTextModel(f32net.F32Net):
    """transformers.CLIPTextModel for SD1.5's text_encoder: `model(input_ids)[0]` is the (b, 77, 768) f32 conditioning"""

    PREFIX = "text_model."
    ANY_DTYPE = True        # the pipeline moves every model with .to(device, dtype=float16): the encoder computes and returns f32 regardless

    def __init__(self, config: Optional[Dict] = None, **kw):
        super().__init__()
        cfg = dict(DEFAULT_CONFIG)
        cfg.update({k: v for k, v in dict(config or {}, **kw).items() if not k.startswith("_")})
        self._check_config(cfg)
        for k in ("architectures", "model_type"):          # what save_pretrained stamps the file with, not a setting
            cfg.pop(k, None)
        self._config = cfg
        self.text_model = _TextTransformer(cfg)
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

    def half(self):
        return self

    def float(self):
        return self

    @classmethod
    def from_config(cls, config: Dict, **kw) -> "CLIPTextModel":
        return cls(config, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, subfolder: Optional[str] = "text_encoder", **_) -> "CLIPTextModel":
        model = cls(modelio.read_config(pretrained_model_path, subfolder))
        model.load_state_dict(modelio.read_state_dict(pretrained_model_path, subfolder, WEIGHT_NAMES))
        return model

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True) -> None:
        modelio.write_folder(save_directory, {"architectures": ["CLIPTextModel"], "model_type": "clip_text_model", **self._config},
                             self.state_dict(), safe_serialization, WEIGHT_NAMES)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """SD1.5's names, with or without the `text_model.` prefix; `embeddings.position_ids` is ignored; a missing or an unknown
        tensor raises KeyError naming it"""
        sd = {(k if k.startswith(self.PREFIX) else self.PREFIX + k): v for k, v in state_dict.items()}
        return super().load_state_dict({k: v for k, v in sd.items() if not k.endswith("embeddings.position_ids")}, strict=True)

    # ---- packing ------------------------------------------------------------------------------------------------------------------
    def _fold(self, sd) -> _Pk:
        """f32 tables and kernel-layout weights, q | k | v fused to one [3C][C] matrix: the token table, the position table, the final
        LayerNorm, then the layers in order.  Nothing here depends on the storage mode."""
        def t(name):
            return sd[self.PREFIX + name].detach().to(torch.float32)

        blocks = []
        for i in range(self._config["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            blocks.append(_Pk(n1_g=t(p + "layer_norm1.weight"), n1_b=t(p + "layer_norm1.bias"),
                              in_w=torch.cat([t(a + f"{n}_proj.weight") for n in "qkv"]), in_b=torch.cat([t(a + f"{n}_proj.bias") for n in "qkv"]),
                              out_w=t(a + "out_proj.weight"), out_b=t(a + "out_proj.bias"),
                              n2_g=t(p + "layer_norm2.weight"), n2_b=t(p + "layer_norm2.bias"),
                              fc1_w=t(p + "mlp.fc1.weight"), fc1_b=t(p + "mlp.fc1.bias"), fc2_w=t(p + "mlp.fc2.weight"), fc2_b=t(p + "mlp.fc2.bias")))
        return _Pk(tok=t("embeddings.token_embedding.weight"), pos=t("embeddings.position_embedding.weight"),
                   lnf_g=t("final_layer_norm.weight"), lnf_b=t("final_layer_norm.bias"), blocks=blocks)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def eos_positions(self, input_ids: torch.Tensor) -> torch.Tensor:
        """row of the pooled output: argmax(input_ids) under SD1.5's legacy eos_token_id == 2, else the first position equal to
        eos_token_id (position 0 when there is none), as transformers does"""
        ids = input_ids.to(torch.int)
        if self._config["eos_token_id"] == 2:
            return ids.argmax(dim=-1)
        return (ids == self._config["eos_token_id"]).int().argmax(dim=-1)

    def encode_ids(self, ids: torch.Tensor, b: int, seq: int, pk: Optional[_Pk] = None) -> torch.Tensor:
        """the launches alone: ids int32 [b * seq] on the device, already checked -> [b * seq, C] after final_layer_norm"""
        pk = self.pack(ids.device) if pk is None else pk
        eps = self._config["layer_norm_eps"]
        x = ops.embed_tokens_f32(ids, pk.tok, pk.pos, b, seq)
        x = f32net.run_blocks(x, pk.blocks, b, seq, self._config["num_attention_heads"], eps, causal=True, act="quick_gelu")
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
