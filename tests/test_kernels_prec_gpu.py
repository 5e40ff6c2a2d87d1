"""Per-kernel parity in BOTH one-pass libraries (-m gpu): libavsd_hip.so (bfloat16) and libavsd_hip_f16.so (IEEE half, the storage of the
per-layer precision plan).  tests/test_ops_gpu.py runs these kernels in bfloat16 only; here every case runs in both builds, on operands
built with ops.to_act, against a float64 statement of the operation on ops.from_act(t).double() — the values the kernel reads.

Bounds (constants of tests/test_tile_choice_gpu.py):
  * 16-bit outputs, rel-L2 over the whole output: bf16 4e-3, fp16 5e-4.  f32 outputs: 2e-5.
  * rel-L2 of EACH output row (attention: each (row, head) slice of d channels; GroupNorm: each (batch, group)): twice the whole-tensor
    bound.  One correct rounding of the result cannot exceed 2^-8 / 2^-11 per element, so the per-row error of a perfect kernel stays
    below the whole-tensor bound; the factor two leaves the same room for the kernel's internal arithmetic.  A whole-tensor norm dilutes an
    error confined to a few rows (a tail tile, one head).
  * attention kernels round the unnormalised probabilities P to the storage type before P.V (attention.hip, xattn.hip).  Where a float64
    emulation that applies ONLY the roundings the kernel's source documents (tests/attn_prec_ref.py: P in the attentions; q, P and the
    attention output in the fused block) itself exceeds bound / 1.5 on a case's inputs, the bound of that case is 1.5 x the emulation's
    error, computed here — never a number read off the kernel.
  * fp8 attention: the existing 8e-2 (e4m3 keeps 3 mantissa bits); its worst (row, head) slice is printed, not bounded: the per-row
    argument above is about ONE rounding to 16 bits, not about e4m3 operands.

Every test prints a `kernels_prec {...}` line with what it measured; tests/golden/kernels_prec_measured.json is a record of those lines
from an MI355X run (a record, not a bound).
"""
import json

import pytest
import torch
import torch.nn.functional as F

from tests import attn_prec_ref as R
from tests.test_blocks_gpu import prec  # noqa: F401  (fixture)
from tests.test_tile_choice_gpu import TOL_F32, act, dev, packed, rel_l2, rndf, tol16

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)]

TOL_FP8 = 8e-2      # tests/test_ops_gpu.py


def worst_row(out, ref, width):
    """largest rel-L2 over the slices of `width` consecutive elements"""
    e, r = (out.double() - ref).reshape(-1, width), ref.reshape(-1, width)
    return (e.norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)).max().item()


def report(kernel, case, prec, **figures):
    print("kernels_prec " + json.dumps({"kernel": kernel, "case": str(case), "prec": prec, **{k: float(f"{v:.4g}") for k, v in figures.items()}}))


def check16(kernel, case, prec, out, ref, width, bound=None, emulation=None):
    """whole-tensor and per-row bounds of a 16-bit output; prints before it asserts"""
    from asva_amd import precision as P

    assert out.dtype == P.ACT and out.shape == ref.shape
    bound = tol16(prec) if bound is None else bound
    whole, row = rel_l2(out, ref), worst_row(out, ref, width)
    extra = {} if emulation is None else {"emulation": emulation}
    report(kernel, case, prec, whole=whole, row=row, bound=bound, **extra)
    assert whole < bound and row < 2 * bound, (whole, row, bound)


def check32(kernel, case, prec, out, ref, width):
    assert out.dtype == torch.float32 and out.shape == ref.shape
    whole, row = rel_l2(out, ref), worst_row(out, ref, width)
    report(kernel, case + " f32", prec, whole=whole, row=row, bound=TOL_F32)
    assert whole < TOL_F32 and row < 2 * TOL_F32, (whole, row)


@pytest.fixture
def ops(prec):
    from asva_amd import ops as _ops

    return _ops


@pytest.fixture
def krot_off(ops):
    """the unrotated K walk: same f32 order as the LDS-direct tiles"""
    ops.set_krot(False)
    yield
    ops.set_krot(True)


# ---- normalisation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nb,rows,c1,c2,groups,silu", [
    (2, 192, 1280, 640, 32, True),       # a group straddles the two sources (60 channels per group)
    (3, 50, 32, 0, 8, True),             # 4 channels per group: a vector holds two whole groups
    (24, 64, 640, 0, 32, False),
    (2, 192, 640, 320, 32, True),        # 30 channels per group
    (2, 3072, 640, 0, 32, True),         # refused by the one-launch form: stats + apply either way
    (24, 1024, 320, 0, 32, False),       # the 960-thread one-launch form
])
def test_groupnorm(ops, prec, nb, rows, c1, c2, groups, silu, fused, monkeypatch):
    monkeypatch.setattr(ops, "_GN_FUSED", fused)
    # sources and output are column slices of wider buffers (ld > channels)
    x1 = ops.to_act(rndf(nb * rows, c1 + 16, seed=1, shift=0.5))[:, 8:8 + c1]
    x2 = ops.to_act(rndf(nb * rows, c2 + 8, seed=2, scale=2.0))[:, :c2] if c2 else None
    C = c1 + c2
    gamma, beta = rndf(C, seed=3, shift=1.0), rndf(C, seed=4)
    buf = torch.zeros(nb * rows, C + 8, dtype=x1.dtype, device=dev())
    out = ops.groupnorm(x1, x2, nb, rows, groups, gamma, beta, 1e-5, silu, out=buf[:, :C])
    assert not buf[:, C:].any()
    x = torch.cat([ops.from_act(x1), ops.from_act(x2)], 1) if c2 else ops.from_act(x1)
    ref = F.group_norm(x.double().reshape(nb, rows, C).permute(0, 2, 1), groups, gamma.double(), beta.double(), 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(nb * rows, C)
    # each (batch, group) separately: a wrong group boundary inside a straddling vector would hide in the whole-tensor norm
    cg = C // groups
    sq = lambda t: (t ** 2).reshape(nb, rows, groups, cg).sum((1, 3)).sqrt()      # noqa: E731
    whole, grp = rel_l2(out, ref), float((sq(out.double() - ref) / sq(ref)).max())
    report("groupnorm", (nb, rows, c1, c2, groups, silu, "fused" if fused else "pair"), prec, whole=whole, row=grp, bound=tol16(prec))
    assert whole < tol16(prec) and grp < 2 * tol16(prec)


@pytest.mark.parametrize("M,C", [(257, 640), (33, 80), (64, 1280), (16, 2048)])
def test_layernorm(ops, prec, M, C):
    x, xv = act(M, C, seed=1, scale=3.0, shift=1.0)
    g, b = rndf(C, seed=2, shift=1.0), rndf(C, seed=3)
    out = ops.layernorm(x, g, b, 1e-5)
    check16("layernorm", (M, C), prec, out, F.layer_norm(xv, (C,), g.double(), b.double(), 1e-5), C)


def test_layernorm_with_frame_pos(ops, prec):
    B, Fr, hw, C = 2, 12, 16, 320
    x, xv = act(B * Fr * hw, C, seed=1)
    pos = rndf(Fr, C, seed=2)
    g, b = rndf(C, seed=3, shift=1.0), rndf(C, seed=4)
    out = ops.layernorm(x, g, b, 1e-5, pos=pos, hw=hw, frames=Fr)
    xp = xv.reshape(B, Fr, hw, C) + pos.double()[None, :, None, :]
    check16("layernorm", ("pos", B, Fr, hw, C), prec, out, F.layer_norm(xp, (C,), g.double(), b.double(), 1e-5).reshape(-1, C), C)


def test_softmax_rows(ops, prec):
    s = rndf(300, 1024, seed=1, scale=4.0)
    check16("softmax_rows", (300, 1024), prec, ops.softmax_rows(s), torch.softmax(s.double(), -1), 1024)


# ---- attention -------------------------------------------------------------------------------------------------------------------------
def heads_of(x, n, heads):
    """[n * L, heads * d] float64 -> [n, heads, L, d]"""
    return x.reshape(n, -1, heads, x.shape[-1] // heads).transpose(1, 2)


def rows_of(o):
    """[n, heads, L, d] -> [n * L, heads * d]"""
    return o.transpose(1, 2).reshape(-1, o.shape[1] * o.shape[3])


def check_attention(kernel, case, prec, out, qh, kh, vh, mask=None, rounded_sum=False):
    """qh / kh / vh [n, heads, L, d] float64 of what the kernel reads.  The bound follows the emulation rule of the module docstring:
    attn_kernel takes its denominator from the ROUNDED probabilities when the head dimension leaves a spare padded row (d % 32 != 0)."""
    from asva_amd import precision as P

    d = qh.shape[-1]
    ref = rows_of(R.sdpa64(qh, kh, vh, mask=mask))
    e_emu = rel_l2(rows_of(R.emulate(qh, kh, vh, P.ACT, mask=mask, rounded_sum=rounded_sum)), ref)
    check16(kernel, case, prec, out, ref, d, bound=R.bound16(P.ACT, e_emu), emulation=e_emu)
    return ref


@pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
@pytest.mark.parametrize("Lq,Lk", [(64, 64), (200, 77)])
def test_attention_first_frame_layout(ops, prec, d, Lq, Lk):
    heads, B, Fr = 4, 2, 3
    C = heads * d
    q, qv = act(B * Fr * Lq, C, seed=1)
    kv, kvv = act(B * Lk, 2 * C, seed=2)          # fused k | v rows, one set per clip
    out = ops.attention(q, kv[:, :C], kv[:, C:], bq=B * Fr, lq=Lq, lk=Lk, kv_rows=Lk, heads=heads, q_per_kv=Fr, frames=Fr)
    per_frame = lambda t: heads_of(t, B, heads).repeat_interleave(Fr, 0)      # noqa: E731
    check_attention("attention", (d, Lq, Lk), prec, out, heads_of(qv, B * Fr, heads), per_frame(kvv[:, :C]), per_frame(kvv[:, C:]),
                    rounded_sum=d % 32 != 0)


def test_attention_key_gather_matches_bool_mask(ops, prec):
    """audio cross-attention: 229 keys, the per-frame gather of 25 against the boolean mask of the reference"""
    from asva_amd.conditioning import audio_segment_mask, mask_to_key_index

    heads, d, B, Fr, Lq = 8, 40, 2, 12, 64
    C = heads * d
    q, qv = act(B * Fr * Lq, C, seed=1)
    k, kvl = act(B * 229, C, seed=2)
    v, vvl = act(B * 229, C, seed=3)
    mask = audio_segment_mask(Fr)                                  # [Fr, 229] bool
    idx = mask_to_key_index(mask).to(dev())                        # [Fr, 25] int32
    assert idx.shape == (Fr, 25)
    out = ops.attention(q, k, v, bq=B * Fr, lq=Lq, lk=25, kv_rows=229, heads=heads, q_per_kv=Fr, frames=Fr, key_index=idx)
    per_frame = lambda t: heads_of(t, B, heads).repeat_interleave(Fr, 0)      # noqa: E731
    m = mask.to(dev()).repeat(B, 1)[:, None, None, :]              # [B * Fr, 1, 1, 229]
    check_attention("attention", ("gather", d, Lq, 229, 25), prec, out, heads_of(qv, B * Fr, heads), per_frame(kvl), per_frame(vvl), mask=m,
                    rounded_sum=True)


@pytest.mark.parametrize("d", [40, 64])
def test_attention_online_softmax_rescale(ops, prec, d):
    """keys far above the rest in LATER tiles force the (rare, deferred) running-max rescale: one spike on each half of the wave, each
    aimed at a different query"""
    Lq, Lk = 32, 160
    qf, kf = rndf(Lq, d, seed=1), rndf(Lk, d, seed=2)
    q = ops.to_act(qf)
    qv = ops.from_act(q).double()
    kf[70], kf[97], kf[130] = ops.from_act(q)[5] * 4, ops.from_act(q)[11] * 6, ops.from_act(q)[5] * 8
    k = ops.to_act(kf)
    v, vv = act(Lk, d, seed=3)
    out = ops.attention(q, k, v, bq=1, lq=Lq, lk=Lk, kv_rows=Lk, heads=1, q_per_kv=1, frames=1)
    ref = check_attention("attention", ("rescale", d), prec, out, qv[None, None], ops.from_act(k).double()[None, None], vv[None, None],
                          rounded_sum=d % 32 != 0)
    assert (out.double() - ref).abs().max() < 0.05      # no row is left at a stale scale


@pytest.mark.parametrize("d", [40, 64])
def test_attention_slowly_growing_max(ops, prec, d):
    """the row maximum creeps up by less than the rescale threshold per tile: the stale-max path must stay exact"""
    Lq, Lk = 64, 256
    q, qv = act(Lq, d, seed=1)
    k = ops.to_act(rndf(Lk, d, seed=2) * torch.linspace(0.5, 3.0, Lk, device=dev())[:, None])
    v, vv = act(Lk, d, seed=3)
    out = ops.attention(q, k, v, bq=1, lq=Lq, lk=Lk, kv_rows=Lk, heads=1, q_per_kv=1, frames=1)
    check_attention("attention", ("slow max", d), prec, out, qv[None, None], ops.from_act(k).double()[None, None], vv[None, None],
                    rounded_sum=d % 32 != 0)


@pytest.mark.parametrize("L", [200, 77])
def test_attention_single_wide_head_512(ops, prec, L):
    """attn_wide_kernel (the VAE mid-block attention): one head over all 512 channels; q | k | v as strided views of one projection"""
    n, C = 3, 512
    qkv, f = act(n * L, 3 * C, seed=1, scale=0.5)
    out = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], bq=n, lq=L, lk=L, kv_rows=L, heads=1, q_per_kv=1, frames=1)
    f = f.reshape(n, 1, L, 3, C)
    check_attention("attention_wide", (512, L), prec, out, f[..., 0, :], f[..., 1, :], f[..., 2, :])


@pytest.mark.parametrize("dom", [0, 700])
def test_attention_probability_tail_below_fp16_normal_range(ops, prec, dom):
    """One key 12 bits above the median score of the 1023 others, with v = 0: the output is made of probabilities at 2^-12 of the row
    maximum (about 22 % of the mass), which IEEE half holds as numbers near and below its smallest normal (2^-14).  A kernel whose P.V
    product loses subnormal P is wrong by 3e-2 here (tests/test_kernels_prec_cpu.py pins that on the reference alone); the emulation
    with gradual underflow costs 3.1e-4 (fp16) / 2.4e-3 (bf16), so the whole-tensor bounds 5e-4 / 4e-3 stay in force.
    dom = 0: the maximum is known from the first tile; dom = 700: it arrives late, through the running-max rescale."""
    from asva_amd import precision as P

    q, k, v = (ops.to_act(t.to(dev())) for t in R.tail_operands(dom))
    out = ops.attention(q, k, v, bq=1, lq=R.TAIL_LQ, lk=R.TAIL_LK, kv_rows=R.TAIL_LK, heads=1, q_per_kv=1, frames=1)
    f = R.tail_figures(ops.from_act(q), ops.from_act(k), ops.from_act(v), dom, P.ACT)
    bound = R.bound16(P.ACT, f["e_grad"])
    assert bound == tol16(prec) and f["tail_mass"] >= 0.15
    report("attention tail figures", ("dom", dom), prec, e_ideal=f["e_ideal"], e_grad=f["e_grad"], e_flush=f["e_flush"], tail_mass=f["tail_mass"])
    check16("attention", ("tail", "dom", dom), prec, out, f["ref"], R.TAIL_D, bound=bound, emulation=f["e_grad"])


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("Fr", [4, 12, 24])
def test_temporal_attention(ops, prec, d, Fr):
    """tattn_kernel: f32 VALU math on the 16-bit rows, no rounding of P — the plain bounds"""
    heads, B, hw = 8, 2, 24
    if heads * Fr > 256:
        heads = 256 // Fr
    C = heads * d
    qkv, f = act(B * Fr * hw, 3 * C, seed=1)
    out = ops.temporal_attention(qkv, b=B, frames=Fr, hw=hw, heads=heads)
    x = f.reshape(B, Fr, hw, 3, heads, d).permute(3, 0, 2, 4, 1, 5)          # [3, B, hw, heads, Fr, d]
    ref = R.sdpa64(x[0], x[1], x[2]).permute(0, 3, 1, 2, 4).reshape(B * Fr * hw, C)
    check16("temporal_attention", (d, Fr), prec, out, ref, d)


@pytest.mark.parametrize("d,heads", [(40, 8), (128, 4)])
@pytest.mark.parametrize("case", ["text", "audio_gather"])
def test_attention_fp8(ops, prec, d, heads, case):
    """avsd_attention_fp8 (the 16-bit -> e4m3 loaders differ between the builds) against float64: text cross-attention (77 keys) and the
    audio key gather (25 of 229 keys per frame)"""
    B, Fr, C, L = 2, 3, d * heads, 160
    if case == "text":
        lk, kv_rows, idx = 77, 77, None
    else:
        lk, kv_rows = 25, 229
        g = torch.Generator().manual_seed(5)
        idx = torch.stack([torch.randperm(229, generator=g)[:lk].sort().values for _ in range(Fr)]).to(torch.int32).to(dev())
    q, qv = act(B * Fr * L, C, seed=1)
    k, kvl = act(B * kv_rows, C, seed=2)
    v, vvl = act(B * kv_rows, C, seed=3)
    o8 = ops.attention(q, k, v, fp8=(1.0, 1.0, 1.0), bq=B * Fr, lq=L, lk=lk, kv_rows=kv_rows, heads=heads, q_per_kv=Fr, frames=Fr, key_index=idx)
    qh = heads_of(qv, B * Fr, heads).reshape(B, Fr, heads, L, d)
    kh, vh = heads_of(kvl, B, heads), heads_of(vvl, B, heads)
    sel = [idx[f].long() if idx is not None else torch.arange(lk, device=dev()) for f in range(Fr)]
    ref = torch.stack([R.sdpa64(qh[:, f], kh[:, :, sel[f]], vh[:, :, sel[f]]) for f in range(Fr)], 1)          # [B, Fr, heads, L, d]
    ref = rows_of(ref.reshape(B * Fr, heads, L, d))
    whole, row = rel_l2(o8, ref), worst_row(o8, ref, d)
    report("attention_fp8", (d, heads, case), prec, whole=whole, row=row, bound=TOL_FP8)
    assert o8.dtype == q.dtype and whole < TOL_FP8


# ---- fused cross-attention block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32_res", [False, True])
@pytest.mark.parametrize("kind,lk,per_frame", [("audio", 25, True), ("text", 77, False)])
def test_cross_attention_block(ops, prec, kind, lk, per_frame, f32_res):
    """avsd_cross_attention_block against the float64 statement res + to_out(softmax(LN(h) Wq K^T / sqrt d) V) on the operands the kernel
    reads (the gain-folded, rounded Wq with its column sums and folded bias), and against the emulation that rounds q, P and the attention
    output to the storage type where xattn.hip does.  C = 320, 8 heads of 40, 2 clips x 3 frames x 256 rows."""
    from asva_amd import precision as P
    from tests.helpers import xattn_block_operands

    p = xattn_block_operands(ops, P.ACT, lk, per_frame, f32_res)
    M, C, heads = p.M, p.C, p.heads
    stats_out = torch.empty_like(p.stats)
    master = torch.empty(M, C, device=dev()) if f32_res else None
    out = ops.cross_attention_block(p.h, p.stats, p.wq_f, p.q_colsum, p.q_bias, p.k_pad, p.vt_pad, lk, p.wo, p.bo, res=p.res, heads=heads, L=p.L,
                                    q_per_kv=p.q_per_kv, rowstats=stats_out, master=master)
    hv, res = p.h.double(), p.res.double()
    norm = (hv - hv.mean(-1, keepdim=True)) * torch.rsqrt(hv.var(-1, unbiased=False, keepdim=True) + 1e-5)
    kv_of = torch.arange(p.B * p.Fr, device=dev()) // p.q_per_kv
    kh, vh = heads_of(p.kk.double()[kv_of].reshape(-1, C), p.B * p.Fr, heads), heads_of(p.vv.double()[kv_of].reshape(-1, C), p.B * p.Fr, heads)
    wo, bo = p.wo.double(), p.bo.double()

    def block(rnd, attn):
        q = rnd(norm @ p.wq_f.double().T + p.q_bias.double())
        return rnd(rows_of(attn(heads_of(q, p.B * p.Fr, heads), kh, vh))) @ wo.T + bo + res

    r16 = lambda t: R.round16(t, P.ACT)                              # noqa: E731
    ref = block(lambda t: t, R.sdpa64)
    emu = r16(block(r16, lambda q, k, v: R.emulate(q, k, v, P.ACT, round_out=False)))      # ... and the one rounding of the output
    tol = tol16(prec)
    e_emu = rel_l2(emu, ref)
    check16("cross_attention_block", (kind, lk, "f32 res" if f32_res else "16-bit res"), prec, out, ref, C, bound=R.bound16(P.ACT, e_emu), emulation=e_emu)
    # attention-only part: subtracting the residual leaves to_out(attention) (the residual dominates `out`)
    e_att, e_att_emu = rel_l2(out.double() - res, ref - res), rel_l2(emu - res, ref - res)
    b_att = 2.5e-2 if prec == "bf16" else R.bound16(P.ACT, e_att_emu)
    report("cross_attention_block", (kind, lk, "f32 res" if f32_res else "16-bit res", "attention only"), prec, whole=e_att, bound=b_att, emulation=e_att_emu)
    assert e_att < b_att
    ob = out.float().reshape(M, C // 32, 32)
    assert torch.allclose(stats_out[..., 0], ob.sum(-1), atol=1e-3, rtol=1e-5) and torch.allclose(stats_out[..., 1], (ob * ob).sum(-1), atol=1e-2, rtol=1e-5)
    if f32_res:
        assert rel_l2(master.to(P.ACT), out) < 1e-6 and rel_l2(master, ref) < tol


# ---- layout, post-processing, copies: bit-exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [False, True])
def test_xattn_pack_kv_matches_indexing(ops, prec, gather):
    from asva_amd.conditioning import audio_segment_mask, mask_to_key_index

    n_kv, C, Fr = 2, 320, 12
    rows = 229 if gather else 77
    kv, _ = act(n_kv * rows, 2 * C, seed=5)
    idx = mask_to_key_index(audio_segment_mask(Fr)).to(dev()) if gather else None
    lk = idx.shape[1] if gather else rows
    nb = n_kv * Fr if gather else n_kv
    lkp = (lk + 31) // 32 * 32
    k = torch.full((nb, lkp, C), float("nan"), dtype=kv.dtype, device=dev())      # poisoned: the launch owns the padding too
    vt = torch.full((nb, C, lkp), float("nan"), dtype=kv.dtype, device=dev())
    ops.xattn_pack_kv(kv, n_kv, rows, C, idx, k, vt)
    kv3 = kv.view(n_kv, rows, 2 * C)
    if gather:
        kv3 = kv3[:, idx.long()].reshape(nb, lk, 2 * C)
    assert torch.equal(k[:, :lk], kv3[..., :C]) and torch.equal(vt[:, :, :lk], kv3[..., C:].transpose(1, 2))
    assert not k[:, lk:].any() and not vt[:, :, lk:].any()


def test_layout_roundtrip_and_replication(ops, prec):
    from asva_amd import precision as P

    B, C, Fr, H, W = 2, 4, 3, 8, 8
    x = rndf(B, C, Fr, H, W, seed=1)
    rows = ops.ncfhw_to_rows(x, cpad=8, rep=2, scale=0.5)
    ref = (0.5 * x).permute(0, 2, 3, 4, 1).reshape(-1, C).to(P.ACT)
    n = B * Fr * H * W
    assert rows.dtype == P.ACT and rows.shape == (2 * n, 8)
    assert torch.equal(rows[:n, :C], ref) and torch.equal(rows[n:, :C], ref)
    assert torch.count_nonzero(rows[:, C:]) == 0
    r32 = rndf(n, 8, seed=2)
    assert torch.equal(ops.rows_to_ncfhw(r32, B, C, Fr, H, W), r32[:, :C].reshape(B, Fr, H, W, C).permute(0, 4, 1, 2, 3))


def test_vae_postprocess(ops, prec):
    n, H, W = 3, 16, 8
    rows, _ = act(n * H * W, 4, seed=1)
    u8 = ops.vae_postprocess_u8(rows, n, H, W)
    want = ((rows[:, :3].float().reshape(n, H, W, 3) / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    assert u8.dtype == torch.uint8 and torch.equal(u8, want)
    out = ops.vae_postprocess(rows, n, H, W)
    assert torch.allclose(out, (rows[:, :3].float().reshape(n, H, W, 3).permute(0, 3, 1, 2) / 2 + 0.5).clamp(0, 1), atol=1e-6)


def test_copy_and_replicate(ops, prec):
    x, _ = act(96, 40, seed=1)
    assert torch.equal(ops.copy(x, rep=3), torch.cat([x] * 3))
    f = rndf(24, 3, 8, seed=2)
    dst = torch.empty(48, 3, 8, device=dev())
    ops.copy(f, dst, rep=2)
    assert torch.equal(dst, torch.cat([f, f]))
    with pytest.raises(ValueError):
        ops.copy(x[:, :8])                       # not contiguous
    with pytest.raises(ValueError):
        ops.copy(act(3, 3, seed=3)[0])           # 18 bytes: not a multiple of 16


# ---- GEMM-family kernels not launched by tile id in IEEE half elsewhere ---------------------------------------------------------------------
def _conv_case(ops, n_img, hs, ws, cin, cout):
    from asva_amd.weights import pack_conv3x3

    M = n_img * hs * ws
    x, xv = act(M, cin, seed=1)
    wf = rndf(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    b = rndf(cout, seed=3)
    res, rv = act(M, cout, seed=4)
    _, wq = packed(wf)
    ref = F.conv2d(xv.reshape(n_img, hs, ws, cin).permute(0, 3, 1, 2), wq, b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    return x, pack_conv3x3(wf), b, res, ref, rv


def _check_resident_conv(ops, prec, tile, shape, split):
    """16-bit output with the full epilogue against float64; the f32 output against float64 and against the tap-major tile 9 (same
    products, another f32 order: tolerance, as tests/test_ops_gpu.py), and bit-identical run to run"""
    n_img, hs, ws, cin, cout = shape
    x, wp, b, res, ref, rv = _conv_case(ops, *shape)
    kw = dict(bias=b, mode=ops.CONV3, conv=(n_img, hs, ws, 1, 0))
    out = ops.gemm(x, wp, res1=res, tile=tile, split_k=split, **kw)
    check16(f"conv3r tile {tile}", (*shape, split), prec, out, ref + rv, cout)
    o32 = ops.gemm(x, wp, out_f32=True, tile=tile, split_k=split, **kw)
    check32(f"conv3r tile {tile}", str((*shape, split)), prec, o32, ref, cout)
    o9 = ops.gemm(x, wp, out_f32=True, tile=9, **kw)
    report(f"conv3r tile {tile}", (*shape, split, "vs tile 9"), prec, whole=rel_l2(o32, o9), bit_equal=float(torch.equal(o32, o9)))
    assert rel_l2(o32, o9) < TOL_F32
    assert torch.equal(o32, ops.gemm(x, wp, out_f32=True, tile=tile, split_k=split, **kw))


@pytest.mark.parametrize("tile", [40, 42, 43, 44, 48])
@pytest.mark.parametrize("n_img,hs,ws,cin,cout,split", [(2, 32, 32, 320, 192, 1), (7, 8, 8, 192, 128, 3), (5, 16, 16, 128, 132, 2)])
def test_gemm_conv3_resident(ops, prec, n_img, hs, ws, cin, cout, split, tile):
    """conv3r.hip: the 3x3 stride-1 convolution with the input tile resident in LDS (bands of image rows / whole images per tile)"""
    from asva_amd import _lib

    if _lib.lib().avsd_gemm_conv3r_supported(tile, hs, ws, cin) == 0:
        pytest.skip("geometry refused by this tile (the refusal itself: tests/test_ops_gpu.py)")
    _check_resident_conv(ops, prec, tile, (n_img, hs, ws, cin, cout), split)


@pytest.mark.parametrize("tile", [51, 52, 53, 54])
@pytest.mark.parametrize("n_img,hs,ws,cin,cout,split", [(2, 64, 64, 64, 128, 1), (2, 12, 64, 64, 64, 1)])
def test_gemm_conv3_resident_2d(ops, prec, n_img, hs, ws, cin, cout, split, tile):
    """conv3r.hip, rectangular tiles (TH image rows x 32 pixels): every border and corner of the zero-filled halo; height 12 admits the
    4-row tile only"""
    from asva_amd import _lib

    if _lib.lib().avsd_gemm_conv3r2d_supported(tile, hs, ws, cin) == 0:
        pytest.skip("geometry refused by this tile (the refusal itself: tests/test_ops_gpu.py)")
    _check_resident_conv(ops, prec, tile, (n_img, hs, ws, cin, cout), split)


@pytest.mark.parametrize("M,N,K", [(1000, 2560, 320), (130, 64, 640)])
def test_gemm_nstream_tile(ops, prec, M, N, K, krot_off):
    """csrc/nstream.hip (tile 70): plain + residual against float64, the f32 output bit-identical to the LDS-direct tile 9; GEGLU with the
    LayerNorm fold against float64 and tile 9"""
    from asva_amd.weights import pack_frag, pack_geglu

    a, av = act(M, K, seed=1)
    w, wv = act(N, K, seed=2, scale=K ** -0.5)
    bias = rndf(N, seed=3)
    res, rv = act(M, N, seed=4)
    wf = pack_frag(w)
    out = ops.gemm(a, w, bias=bias, res1=res, tile=70, w_frag=wf)
    check16("nstream tile 70", (M, N, K), prec, out, av @ wv.T + bias.double() + rv, N)
    assert torch.equal(out, ops.gemm(a, w, bias=bias, res1=res, tile=9))
    o32 = ops.gemm(a, w, bias=bias, out_f32=True, tile=70, w_frag=wf)
    check32("nstream tile 70", str((M, N, K)), prec, o32, av @ wv.T + bias.double(), N)
    assert torch.equal(o32, ops.gemm(a, w, bias=bias, out_f32=True, tile=9))
    # the GEGLU projection as the transformer block runs it: producer statistics -> LayerNorm fold -> value * gelu(gate)
    wp, bp = pack_geglu(w.float(), bias)
    wpf = pack_frag(wp)
    st = torch.empty(M, K // 32, 2, device=dev())
    h = ops.gemm(act(M, K, seed=6)[0], act(K, K, seed=7, scale=K ** -0.5)[0], rowstats=st, tile=9)
    cs = wp.float().sum(1)
    got = ops.gemm(h, wp, bias=bp, geglu=True, ln=(st, cs, 1e-5), tile=70, w_frag=wpf)
    assert torch.equal(got, ops.gemm(h, wp, bias=bp, geglu=True, ln=(st, cs, 1e-5), tile=9))
    hv = h.double()
    y = (hv - hv.mean(1, keepdim=True)) * torch.rsqrt(hv.var(1, unbiased=False, keepdim=True) + 1e-5) @ wv.T + bias.double()
    check16("nstream tile 70", (M, N, K, "GEGLU + LayerNorm fold"), prec, got, y[:, :N // 2] * F.gelu(y[:, N // 2:]), N // 2)


@pytest.mark.parametrize("tile", [61, 62, 63, 64, 65, 66, 67])
@pytest.mark.parametrize("B,hw,C,N", [(1, 32, 128, 132), (3, 96, 64, 64)])
def test_gemm_asm_tiles_tmix(ops, prec, tile, B, hw, C, N, krot_off):
    """csrc/gemm4.hip, the temporal-mix A operand in the hand-scheduled loop (frame 0 -> previous frame -> current frame at the two
    K-segment boundaries), unrotated K walk: full epilogue against float64, the f32 output bit-identical to tile 9"""
    Fr = 12
    M = B * Fr * hw
    y, yv = act(M, C, seed=1)
    w, wv = act(N, 3 * C, seed=2, scale=(3 * C) ** -0.5)
    b, temb = rndf(N, seed=3), rndf(B, N, seed=5)
    res2, r2v = act(M, N, seed=4)
    y4 = yv.reshape(B, Fr, hw, C)
    cat = torch.cat([y4[:, :1].expand_as(y4), torch.cat([y4[:, :1], y4[:, :-1]], 1), y4], -1).reshape(M, 3 * C)
    ref = cat @ wv.T + b.double() + temb.double().repeat_interleave(Fr * hw, 0) + r2v
    kw = dict(bias=b, rowvec=temb, rows_per_vec=Fr * hw, res2=res2, mode=ops.TMIX, tmix=(hw, Fr))
    check16(f"asm tile {tile} TMIX", (B, hw, C, N), prec, ops.gemm(y, w, tile=tile, **kw), ref, N)
    o32 = ops.gemm(y, w, out_f32=True, tile=tile, **kw)
    check32(f"asm tile {tile} TMIX", str((B, hw, C, N)), prec, o32, ref, N)
    assert torch.equal(o32, ops.gemm(y, w, out_f32=True, tile=9, **kw))
