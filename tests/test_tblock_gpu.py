"""avsd_temporal_block (csrc/tblock.hip, -m gpu): the temporal attention of a 320-channel transformer block — LayerNorm(h + pos)-folded
q|k|v projection, softmax attention over the 12 frames of a pixel per head, output projection + h and the row statistics of the result —
as one launch, in both one-pass libraries.

Each case compares the fused output and row statistics with (a) the three launches it replaces (ops.gemm with ln= / ln_pos=,
ops.temporal_attention, ops.gemm with rowstats=) and (b) a float64 evaluation of LayerNorm(h + pos), the projection, the attention and the
output projection + h on the values the kernels read (the packed 16-bit weights) that rounds q|k|v and o to the storage type where the
kernels do.  The bound has no constant of its own: rel_l2(fused, ref) <= 1.25 x rel_l2(separate, ref), the project's bound for a fused
launch (tests/test_ffblock_gpu.py, tests/test_qattn_gpu.py).

The kernel keeps every product's K order ascending in 16-wide steps into one accumulator, runs the attention in tattn_kernel's order and
adds the epilogue terms in the shared epilogue's order, so it is also held to bit identity with the three launches on the LDS-direct tile 9
with the unrotated K walk, output and statistics.

Geometries (B, hw), frames = 12: (1, 8) one exact band of 8 pixel columns; (1, 9) one column into a second band; (2, 12) the middle band
straddles the batch boundary; (2, 16) four full bands."""
import pytest
import torch

from tests.helpers import rel_l2
from tests.test_blocks_gpu import prec  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)]

C, HEADS, D, FR, MMAX = 320, 8, 40, 12, 384
EPS = 1e-5
GEOS = [(1, 8), (1, 9), (2, 12), (2, 16)]


@pytest.fixture
def ops(prec):
    from asva_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


_CACHE: dict = {}


def weights(ops, prec):
    """weights, position table and 384 rows of the projection in front of the block, per precision, built once and never written again"""
    if prec in _CACHE:
        return _CACHE[prec]
    from types import SimpleNamespace

    from asva_amd.weights import group_qkv, pack_frag, to_act

    def rndf(*shape, seed=0, scale=1.0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dev())

    o = SimpleNamespace()
    o.a0 = to_act(rndf(MMAX, C, seed=1))
    o.w0 = to_act(rndf(C, C, seed=2, scale=C ** -0.5))
    o.res0 = to_act(rndf(MMAX, C, seed=3) + 0.5)
    o.pos = 0.5 * rndf(FR, C, seed=13)
    gamma, beta = 1 + 0.1 * rndf(C, seed=4), 0.1 * rndf(C, seed=5)
    w = rndf(3 * C, C, seed=6, scale=2.0 * C ** -0.5)
    o.wqkv_ln = to_act(w * gamma[None, :])                                   # as Packer.lnfold (asva_amd/unet.py)
    o.sqkv, o.bqkv = o.wqkv_ln.float().sum(1), w @ beta
    o.posw = ops.linear_small_m(o.pos, o.wqkv_ln, None)                      # as make_cond_block
    o.wo, o.bo = to_act(rndf(C, C, seed=8, scale=C ** -0.5)), 0.1 * rndf(C, seed=9)
    o.wqkv_f, o.sqkv_f, o.bqkv_f = pack_frag(group_qkv(o.wqkv_ln)), group_qkv(o.sqkv), group_qkv(o.bqkv)
    o.posw_f = group_qkv(o.posw.t()).t().contiguous()
    o.wo_f = pack_frag(o.wo)
    o.geo = {}
    torch.cuda.synchronize()
    _CACHE[prec] = o
    return o


def operands(ops, prec, B, hw):
    """the residual stream h of (B, 12, hw) with the statistics of h + pos[frame], and the float64 reference, per geometry"""
    from types import SimpleNamespace

    from asva_amd import precision as P

    o = weights(ops, prec)
    if (B, hw) in o.geo:
        return o, o.geo[(B, hw)]
    M = B * FR * hw
    g = SimpleNamespace(M=M)
    g.stats = torch.empty(M, C // 32, 2, device=dev())
    g.h = ops.gemm(o.a0[:M], o.w0, res1=o.res0[:M], rowstats=g.stats, stats_pos=(o.pos, hw, FR))
    # float64 on the same values, q|k|v and o rounded to the storage type where the kernels round them
    frame = (torch.arange(M, device=dev()) // hw) % FR
    hv = g.h.double()
    x = hv + o.pos.double()[frame]
    ln = (x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + EPS)
    qkv = (ln @ o.wqkv_ln.double().T + o.bqkv.double()).to(P.ACT).double()
    q, k, v = (t.reshape(B, FR, hw, HEADS, D).permute(0, 2, 3, 1, 4) for t in qkv.split(C, 1))         # [B, hw, heads, frames, d]
    p = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1)
    att = (p @ v).permute(0, 3, 1, 2, 4).reshape(M, C).to(P.ACT).double()
    g.ref = att @ o.wo.double().T + o.bo.double() + hv
    # the statistics of the float64 result itself: the kernels sum the ROUNDED values (AVSD_GEMM_ROWSTATS), so both forms carry the
    # rounding of all 32 values of a block against it — an error that every element feeds, where the statistics of the rounded reference
    # would differ only through the few values that round the other way
    r = g.ref.reshape(M, C // 32, 32)
    g.ref_stats = torch.stack([r.sum(-1), (r * r).sum(-1)], -1)
    torch.cuda.synchronize()
    o.geo[(B, hw)] = g
    return o, g


def fused(ops, o, g, B, hw, h=None, out=None, rowstats=None):
    st = torch.empty(g.M, C // 32, 2, device=dev()) if rowstats is None else rowstats
    out = ops.temporal_block(g.h if h is None else h, g.stats, o.wqkv_f, o.sqkv_f, o.bqkv_f, o.posw_f, o.wo_f, o.bo, b=B, frames=FR, hw=hw,
                             heads=HEADS, eps=EPS, rowstats=st, out=out)
    return out, st


def separate(ops, o, g, B, hw, tile=0):
    """the launches of unet._transformer step 4"""
    qkv = ops.gemm(g.h, o.wqkv_ln, bias=o.bqkv, ln=(g.stats, o.sqkv, EPS), ln_pos=(o.posw, hw, FR), tile=tile)
    att = ops.temporal_attention(qkv, b=B, frames=FR, hw=hw, heads=HEADS)
    st = torch.empty(g.M, C // 32, 2, device=dev())
    return ops.gemm(att, o.wo, bias=o.bo, res1=g.h, rowstats=st, tile=tile), st


@pytest.mark.parametrize("B,hw", GEOS)
def test_temporal_block_matches_separate_launches_and_float64(ops, prec, B, hw):
    from asva_amd import precision as P

    o, g = operands(ops, prec, B, hw)
    out, st = fused(ops, o, g, B, hw)
    assert out.dtype == P.ACT and out.shape == (g.M, C)
    sep, sep_st = separate(ops, o, g, B, hw)
    e_fused, e_sep = rel_l2(out, g.ref), rel_l2(sep, g.ref)
    s_fused, s_sep = rel_l2(st, g.ref_stats), rel_l2(sep_st, g.ref_stats)
    print(f"temporal_block {prec} B={B} hw={hw}: fused vs float64 {e_fused:.4e}, separate vs float64 {e_sep:.4e}, fused vs separate "
          f"{rel_l2(out, sep):.4e}; statistics {s_fused:.4e}, {s_sep:.4e}")
    assert e_fused <= 1.25 * e_sep, (e_fused, e_sep)
    assert s_fused <= 1.25 * s_sep, (s_fused, s_sep)
    # a repeat run is bit-identical
    out2, st2 = fused(ops, o, g, B, hw)
    assert torch.equal(out2, out) and torch.equal(st2, st)
    # every sum in the launches' order: bit-identical to them on the LDS-direct tile 9, unrotated
    ops.set_krot(False)
    try:
        want, want_st = separate(ops, o, g, B, hw, tile=9)
    finally:
        ops.set_krot(True)
    assert torch.equal(out, want)
    assert torch.equal(st, want_st)


@pytest.mark.parametrize("B,hw", [(1, 9), (2, 12)])
def test_temporal_block_padding_and_strides(ops, prec, B, hw):
    """h and out as column slices of wider buffers (ld = C + 16) with rows past M: the padding of h holds 3e4 and never reaches the result;
    columns outside C and rows past M of the output buffer, and statistics rows past M, keep their sentinel"""
    from asva_amd import precision as P

    o, g = operands(ops, prec, B, hw)
    M = g.M
    want, want_st = fused(ops, o, g, B, hw)
    rows = M + 104
    hb = torch.full((rows, C + 16), 3.0e4, dtype=P.ACT, device=dev())
    hb[:M, 8:8 + C] = g.h
    ob = torch.full((rows, C + 16), 7.0, dtype=P.ACT, device=dev())
    sb = torch.full((rows, C // 32, 2), 7.0, device=dev())
    got, got_st = fused(ops, o, g, B, hw, h=hb[:M, 8:8 + C], out=ob[:M, 8:8 + C], rowstats=sb[:M])
    assert torch.equal(got, want) and torch.equal(got_st, want_st)
    assert bool((ob[:, :8] == 7.0).all()) and bool((ob[:, 8 + C:] == 7.0).all()) and bool((ob[M:] == 7.0).all())
    assert bool((sb[M:] == 7.0).all())


def test_temporal_block_refuses_what_is_not_built(ops, prec):
    from asva_amd import _lib
    from asva_amd import precision as P

    B, hw = 1, 8
    o, g = operands(ops, prec, B, hw)
    M = g.M
    z16 = lambda *s: torch.zeros(*s, dtype=P.ACT, device=dev())         # noqa: E731
    z32 = lambda *s: torch.zeros(*s, device=dev())                      # noqa: E731
    sentinel = lambda *s: torch.full(s, 7.0, dtype=P.ACT, device=dev())  # noqa: E731

    def refused(call, out):
        with pytest.raises(_lib.AvsdError, match=r"avsd_temporal_block failed \(code -1\): temporal_block: unsupported"):
            call(out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())          # AVSD_EINVAL: nothing was launched

    big = 1 << 20
    assert not ops.temporal_block_supported(big, 640, 8, FR) and not ops.temporal_block_supported(big, 1280, 16, FR)
    assert not ops.temporal_block_supported(big, C, 4, FR) and not ops.temporal_block_supported(big, C, HEADS, 24)
    assert not ops.temporal_block_supported(0, C, HEADS, FR) and not ops.temporal_block_supported(96, C, HEADS, FR)     # below break-even
    # C = 640
    C2, nq2 = 640, 1920
    refused(lambda out: ops.temporal_block(z16(M, C2), z32(M, C2 // 32, 2), z16(nq2 // 32, C2 // 16, 64, 8), z32(nq2), z32(nq2), z32(FR, nq2),
                                           z16(C2 // 32, C2 // 16, 64, 8), z32(C2), b=B, frames=FR, hw=hw, heads=8, out=out), sentinel(M, C2))
    # 4 heads; 24 frames (cfg 4)
    refused(lambda out: ops.temporal_block(g.h, g.stats, o.wqkv_f, o.sqkv_f, o.bqkv_f, o.posw_f, o.wo_f, o.bo, b=B, frames=FR, hw=hw, heads=4,
                                           out=out), sentinel(M, C))
    refused(lambda out: ops.temporal_block(z16(2 * M, C), z32(2 * M, C // 32, 2), o.wqkv_f, o.sqkv_f, o.bqkv_f, z32(24, 1024), o.wo_f, o.bo, b=B,
                                           frames=24, hw=hw, heads=HEADS, out=out), sentinel(2 * M, C))
    # ld = C + 4
    hb = z16(M, C + 4)
    hb[:, :C] = g.h
    refused(lambda out: fused(ops, o, g, B, hw, h=hb[:, :C], out=out), sentinel(M, C))
    ob = sentinel(M, C + 4)
    refused(lambda out: fused(ops, o, g, B, hw, out=out[:, :C]), ob)
    # split precision keeps the three launches
    P.set_split(True)
    try:
        assert not ops.temporal_block_supported(big, C, HEADS, FR)
        with pytest.raises(ValueError, match="not built for split precision"):
            fused(ops, o, g, B, hw)
    finally:
        P.set_split(False)


def _block(M_, prec_name, fuse, B, Fr, H, W, text, audio, x):
    """unet._transformer at C = 320 on (B, Fr, H, W) in the named precision ("bf16x2": split precision), on filler weights"""
    from asva_amd import ops as _ops, precision as P, unet
    from asva_amd.conditioning import audio_segment_mask, mask_to_key_index
    from asva_amd.unet import _Act, _Pk, _Transformer3D
    from tests.test_blocks_gpu import _pack

    P.set_precision("bf16" if prec_name == "bf16x2" else prec_name)
    P.set_split(prec_name == "bf16x2")
    root = _pack(_Transformer3D(C, 768, 768), "blk.tr_320.", "tr")
    idx = mask_to_key_index(audio_segment_mask(Fr)).cuda()
    cond = M_.make_cond_block(root.p, _ops.to_act(text), 1, _ops.to_act(audio), 1, Fr, idx, Fr)
    st = _Pk(B=B, F=Fr, temb=None, temb_rows=Fr, cond=_Pk(blocks=[cond], key_index=idx, idx_frames=Fr, frames=Fr, batch=B), tr_i=0, groups=32,
             eps=1e-5, heads=(8,), fuse_ln=True, f32_stream=False, fp8=None)
    old = unet._FUSE_TATTN
    unet._FUSE_TATTN = fuse
    calls = []
    real = _ops.temporal_block

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    _ops.temporal_block = counted
    try:
        out = M_._transformer(st, _Act(_ops.to_act(x)), root.p, (H, W), 8)
    finally:
        unet._FUSE_TATTN = old
        _ops.temporal_block = real
    assert len(calls) == (1 if fuse else 0)
    return _ops.from_act(out.lo).float()


def test_transformer_block_with_and_without_the_fused_temporal_attention(ops, prec):
    """unet._transformer at C = 320, 12 frames on the smallest geometry ops.temporal_block_supported admits, hook on and off, under the two
    bounds of the kernel cases: the 1.25 x bound on the default K walk and bit identity on the unrotated one.  The reference is
    the same block in split precision (16 significant bits in every stored value), which tests/test_blocks_gpu.py holds to < 2e-5 of the
    reference implementation's fp32 module — two orders below the errors compared here."""
    from asva_amd import precision as P
    from asva_amd.unet import AudioUNet3DConditionModel as M_
    from oracle.filler import seeded_randn_bf16

    geo = next(((B, H, W) for B, H, W in [(1, 32, 64), (1, 48, 64), (2, 48, 64)] if ops.temporal_block_supported(B * FR * H * W, C, HEADS, FR)), None)
    assert geo is not None, "temporal_block_supported admits none of the block-test geometries"
    B, H, W = geo
    x = seeded_randn_bf16(101, B, C, FR, H, W).permute(0, 2, 3, 4, 1).reshape(-1, C).cuda().contiguous()
    text, audio = seeded_randn_bf16(102, B, 77, 768).cuda(), seeded_randn_bf16(103, B, 229, 768).cuda()
    try:
        ref = _block(M_, "bf16x2", False, B, FR, H, W, text, audio, x)
        on = _block(M_, prec, True, B, FR, H, W, text, audio, x)
        off = _block(M_, prec, False, B, FR, H, W, text, audio, x)
        # the unrotated K walk: every tile _transformer picks sums K in ascending order, as the fused launch does
        ops.set_krot(False)
        try:
            on0 = _block(M_, prec, True, B, FR, H, W, text, audio, x)
            off0 = _block(M_, prec, False, B, FR, H, W, text, audio, x)
        finally:
            ops.set_krot(True)
    finally:
        P.set_split(False)
        P.set_precision(prec)
    e_on, e_off = rel_l2(on, ref), rel_l2(off, ref)
    print(f"transformer block {prec} M={B * FR * H * W}: fused temporal attention vs split precision {e_on:.4e}, three launches {e_off:.4e}, "
          f"fused vs three launches {rel_l2(on, off):.4e}")
    assert e_on <= 1.25 * e_off, (e_on, e_off)
    # what _transformer hands the kernel — the statistics of h + pos from the text cross-attention, the regrouped position rows of
    # make_cond_block, the Packer's regrouped weights, column sums and bias — reproduces the three launches bit for bit
    print(f"transformer block {prec}, unrotated K walk: fused vs three launches {rel_l2(on0, off0):.4e}, differing values {int((on0 != off0).sum())}")
    assert torch.equal(on0, off0)
