"""Plain-torch restatement of SD1.5's CLIP text encoder (transformers' CLIPTextModel: embeddings, pre-LN blocks with a causal mask,
quick-GELU, final LayerNorm), in fp32 or float64, and the seeded weight recipe that tools/gen_clip_text_golden.py and the tests share.
tests/test_clip_text_cpu.py pins the restatement to the transformers fixture; the GPU tests lean on it where transformers is absent."""
import math

import torch
import torch.nn.functional as F

SMALL = dict(vocab_size=128, hidden_size=128, intermediate_size=256, num_attention_heads=2, max_position_embeddings=77,
             hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=126, pad_token_id=127)
# net "l1": one layer, pooled row = first position equal to eos_token_id; net "l2": two layers and SD1.5's legacy eos_token_id == 2
# (pooled row = argmax of the ids)
NETS = {"l1": dict(SMALL, num_hidden_layers=1, eos_token_id=127), "l2": dict(SMALL, num_hidden_layers=2, eos_token_id=2)}
SD15 = dict(vocab_size=1024, hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=1022, pad_token_id=1023, eos_token_id=1023)
SEED = 20240811
QK_GAIN = 1.5          # q and k weights ~ N(0, (QK_GAIN / sqrt(C))^2): pre-softmax logits of std ~ QK_GAIN^2 (the 0.02 initialisation gives a
#                        flat softmax, and a masking error would barely move the output)


def state_dict_shapes(cfg):
    """names (without the `text_model.` prefix) and shapes of the encoder's state dict, in a fixed order"""
    c, inter = cfg["hidden_size"], cfg["intermediate_size"]
    s = {"embeddings.token_embedding.weight": [cfg["vocab_size"], c], "embeddings.position_embedding.weight": [cfg["max_position_embeddings"], c]}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"], s[p + f"self_attn.{n}.bias"] = [c, c], [c]
        s[p + "layer_norm1.weight"], s[p + "layer_norm1.bias"] = [c], [c]
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = [inter, c], [inter]
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = [c, inter], [c]
        s[p + "layer_norm2.weight"], s[p + "layer_norm2.bias"] = [c], [c]
    s["final_layer_norm.weight"], s["final_layer_norm.bias"] = [c], [c]
    return s


def draw_state_dict(cfg, seed=SEED, prefix=""):
    """the seeded weights: one generator, tensors drawn in the order of state_dict_shapes"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in state_dict_shapes(cfg).items():
        t = torch.randn(shape, generator=g)
        if "layer_norm" in name:
            t = 1.0 + 0.1 * t if name.endswith("weight") else 0.1 * t
        elif name.endswith("bias"):
            t = 0.1 * t
        elif "position_embedding" in name:
            t = 0.5 * t
        elif "q_proj" in name or "k_proj" in name:
            t = t * (QK_GAIN / math.sqrt(shape[1]))
        elif "token_embedding" not in name:
            t = t / math.sqrt(shape[1])
        sd[prefix + name] = t.contiguous()
    return sd


def _strip(sd):
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}


def forward(sd, cfg, ids, dtype=torch.float32, logits_out=None):
    """ids (b, L) integer -> last_hidden_state (b, L, C) in `dtype`; `logits_out`, if a list, receives the pre-softmax logits of every
    layer at the unmasked positions"""
    sd = {k: v.to(dtype) for k, v in _strip(sd).items() if v.is_floating_point()}
    b, L = ids.shape
    c, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    d = c // heads
    x = sd["embeddings.token_embedding.weight"][ids.long()] + sd["embeddings.position_embedding.weight"][:L]
    keep = torch.ones(L, L, dtype=torch.bool).tril()
    mask = torch.zeros(L, L, dtype=dtype).masked_fill(~keep, float("-inf"))
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        lin = lambda t, n: F.linear(t, sd[p + n + ".weight"], sd[p + n + ".bias"])  # noqa: E731
        h = F.layer_norm(x, (c,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
        q, k, v = (lin(h, f"self_attn.{n}").view(b, L, heads, d).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        logits = (q * d ** -0.5) @ k.transpose(-1, -2)
        if logits_out is not None:
            logits_out.append(logits[:, :, keep])
        a = torch.softmax(logits + mask, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(b, L, c), "self_attn.out_proj")
        h = lin(F.layer_norm(x, (c,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps), "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), "mlp.fc2")
    return F.layer_norm(x, (c,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps)


def eos_positions(cfg, ids):
    """transformers' pooled row: argmax(ids) under the legacy eos_token_id == 2, else the first position equal to eos_token_id"""
    if cfg["eos_token_id"] == 2:
        return ids.int().argmax(-1)
    return (ids.int() == cfg["eos_token_id"]).int().argmax(-1)


def pooled(cfg, ids, last):
    return last[torch.arange(ids.shape[0]), eos_positions(cfg, ids)]


def make_ids(cfg, seed=SEED):
    """id rows of length 77: EOS (the highest id, also the padding after it) at position 1, at 10, at 76 and nowhere, and a batch of 3"""
    g = torch.Generator().manual_seed(seed + 1)
    L, top = cfg["max_position_embeddings"], cfg["vocab_size"] - 1
    rows = {}
    for name, at in (("eos1", 1), ("eos10", 10), ("eos76", 76), ("none", None)):
        r = torch.randint(3, top - 1, (1, L), generator=g)
        r[0, 0] = cfg["bos_token_id"]
        if at is not None:
            r[0, at:] = top
        rows[name] = r
    rows["batch3"] = torch.cat([rows["eos10"], rows["none"], rows["eos1"]])
    return rows


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
