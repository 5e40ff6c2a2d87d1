"""Float64 statements and rounding emulations of the attention kernels, for tests/test_kernels_prec_gpu.py and _cpu.py.  TEST
INFRASTRUCTURE ONLY (runs on any device torch has; the product never imports it).

The attention kernels (asva_amd/csrc/attention.hip, xattn.hip) round the unnormalised probabilities P = exp(s - rowmax) to the 16-bit
storage type before the P.V MFMA.  bfloat16 keeps f32's exponent range; IEEE half turns everything below 2^-14 of the row maximum into a
subnormal and everything below 2^-25 into zero.  `emulate` applies exactly that rounding (and the one rounding of the result) in float64,
with gradual underflow or with subnormals flushed, so a test can tell what the documented roundings cost on ITS inputs — and whether a
kernel does worse than they explain.

`tail_operands` builds the case that separates the two: one dominant key `gap_bits` above the median tail score, with v[dom] = 0, so the
whole output comes from keys whose probabilities sit at 2^-gap_bits of the row maximum.
"""
import math

import torch

TOL16 = {torch.bfloat16: 4e-3, torch.float16: 4e-3 / 8}      # rel-L2 bounds of 16-bit outputs (tests/test_tile_choice_gpu.py)
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}   # smallest normal number of the storage type


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def round16(x, dtype, flush=False):
    """float64 -> nearest value of the 16-bit type -> float64; flush: results below the smallest normal number become zero"""
    r = x.float().to(dtype).double()
    return torch.where(r.abs() < TINY[dtype], torch.zeros_like(r), r) if flush else r


def scores(q, k, scale, mask=None):
    """q [..., Lq, d], k [..., Lk, d] float64 -> scaled scores [..., Lq, Lk]; mask (True = visible) broadcasts over them"""
    s = q @ k.transpose(-1, -2) * scale
    return s if mask is None else s.masked_fill(~mask, float("-inf"))


def sdpa64(q, k, v, scale=None, mask=None):
    """softmax(q k^T scale) v in float64"""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return torch.softmax(scores(q.double(), k.double(), scale, mask), -1) @ v.double()


def emulate(q, k, v, dtype, scale=None, mask=None, flush=False, rounded_sum=False, round_out=True):
    """the same product with P = exp(s - rowmax) rounded to `dtype` before P.V, divided by the sum of the UNROUNDED probabilities (the f32
    psum of the kernels; rounded_sum: by the sum of the rounded ones, as the forms that take the denominator from a row of ones in V^T), and
    the result rounded once"""
    q, k, v = q.double(), k.double(), v.double()
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = scores(q, k, scale, mask)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    pr = round16(p, dtype, flush)
    o = (pr @ v) / (pr if rounded_sum else p).sum(-1, keepdim=True)
    return round16(o, dtype) if round_out else o


def bound16(dtype, e_emulation):
    """the bound of a 16-bit attention output: the whole-tensor bound of the storage type, unless the documented roundings alone cost more
    than bound / 1.5 on these inputs — then 1.5 x what they cost"""
    return max(TOL16[dtype], 1.5 * e_emulation)


# ---- the probability tail below the fp16 normal range ---------------------------------------------------------------------------------
TAIL_D, TAIL_LQ, TAIL_LK = 64, 32, 1024


def tail_operands(dom, gap_bits=12.0, d=TAIL_D, lq=TAIL_LQ, lk=TAIL_LK):
    """f32 (q [lq, d], k [lk, d], v [lk, d]) on the CPU: every query points along one unit vector u, key `dom` = b u scores gap_bits
    powers of two above the median of the others and carries v = 0.  Draw order from ONE generator (seed 1): u, q, k, v."""
    g = torch.Generator(device="cpu").manual_seed(1)
    u = torch.randn(d, generator=g)
    u = u / u.norm()
    q = 4.0 * u + 0.25 * torch.randn(lq, d, generator=g)
    k = 0.5 * torch.randn(lk, d, generator=g)
    k[dom] = gap_bits * math.log(2.0) / (4.0 * d ** -0.5) * u
    v = torch.randn(lk, d, generator=g)
    v[dom] = 0.0
    return q, k, v


def tail_figures(q, k, v, dom, dtype):
    """q, k, v: the values the kernel reads (already rounded to `dtype`).  -> dict: float64 reference, the tail's share of the probability
    mass (mean over the queries), the error of rounding the exact result once, of the emulation with gradual underflow (e_grad) and of
    the emulation with subnormal P flushed to zero"""
    ref = sdpa64(q, k, v)
    p = torch.softmax(scores(q.double(), k.double(), q.shape[-1] ** -0.5), -1)
    return {"ref": ref, "tail_mass": float((1.0 - p[..., dom]).mean()), "e_ideal": rel_l2(round16(ref, dtype), ref),
            "e_grad": rel_l2(emulate(q, k, v, dtype), ref), "e_flush": rel_l2(emulate(q, k, v, dtype, flush=True), ref)}
