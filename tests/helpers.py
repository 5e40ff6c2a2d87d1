"""Shared test helpers: golden loading, filler-weight models, error metrics."""
import json
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def load_golden(name):
    return torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=True)


def load_shapes(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def filled_unet(cfg, dtype=torch.float32, heavy_tail=False):
    """Product model with the closed-form filler weights (oracle/filler.py) — the same weights the
    reference model had when the golden vectors were generated."""
    from asva_amd.unet import AudioUNet3DConditionModel
    from oracle.filler import fill_module_

    m = AudioUNet3DConditionModel.from_config(cfg).eval()
    # the SD1.5-shaped model is filled a dozen times per session (1.17 B values from a single-threaded generator, ~5 s each):
    # keep the last filled state_dict of a configuration and copy it
    key = (json.dumps(dict(cfg), sort_keys=True, default=str), bool(heavy_tail))
    if _FILLED.get("key") == key:
        m.load_state_dict(_FILLED["sd"])
    else:
        fill_module_(m, heavy_tail=heavy_tail)
        if sum(p.numel() for p in m.parameters()) > 100_000_000:
            _FILLED.clear()
            _FILLED.update(key=key, sd={k: v.detach().clone() for k, v in m.state_dict().items()})
    return m.to(dtype)


_FILLED: dict = {}


def bf16_round_state_dict(sd):
    return {k: v.to(torch.bfloat16).float() if v.dim() >= 2 else v.float() for k, v in sd.items()}


def xattn_block_operands(ops, dtype, lk, per_frame, f32_res, B=2, Fr=3, L=256, C=320, heads=8):
    """Operands of avsd_cross_attention_block in the 16-bit storage type `dtype` (the active precision's), as a namespace: the residual stream
    h with its LayerNorm statistics (from a ROWSTATS producer GEMM), the gain-folded Q projection, padded K / V^T of `lk` keys (one set per
    frame or per clip), the output projection, and the residual the block adds (h itself, or an f32 master that differs from it)."""
    from types import SimpleNamespace

    dev = torch.device("cuda:0")

    def rndf(*shape, seed=0, scale=1.0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    def rnd(*shape, seed=0, scale=1.0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)

    o = SimpleNamespace(B=B, Fr=Fr, L=L, C=C, heads=heads, d=C // heads, M=B * Fr * L, lk=lk)
    a0 = rnd(o.M, C, seed=1)
    w0 = rnd(C, C, seed=2, scale=C ** -0.5)
    res0 = rnd(o.M, C, seed=3) + 0.5
    o.stats = torch.empty(o.M, C // 32, 2, device=dev)
    o.h = ops.gemm(a0, w0, res1=res0, rowstats=o.stats)                     # residual stream + its LayerNorm statistics
    o.gamma, o.beta = 1 + 0.1 * rndf(C, seed=4), 0.1 * rndf(C, seed=5)
    o.wq = rndf(C, C, seed=6, scale=C ** -0.5)
    o.wq_f = (o.wq * o.gamma[None, :]).to(dtype)
    o.q_colsum, o.q_bias = o.wq_f.float().sum(1), o.wq @ o.beta
    o.wo, o.bo = rnd(C, C, seed=7, scale=C ** -0.5), rndf(C, seed=8)
    o.nkv = B * Fr if per_frame else B
    lkp = (lk + 31) // 32 * 32
    o.kk, o.vv = rnd(o.nkv, lk, C, seed=9), rnd(o.nkv, lk, C, seed=10)
    o.k_pad = torch.zeros(o.nkv, lkp, C, dtype=dtype, device=dev)
    o.vt_pad = torch.zeros(o.nkv, C, lkp, dtype=dtype, device=dev)
    o.k_pad[:, :lk] = o.kk
    o.vt_pad[:, :, :lk] = o.vv.transpose(1, 2)
    o.q_per_kv = 1 if per_frame else Fr
    o.master_in = o.h.float() + 1e-3 * rndf(o.M, C, seed=11) if f32_res else None      # an f32 master that differs from its 16-bit copy
    o.res = o.master_in if f32_res else o.h
    return o
