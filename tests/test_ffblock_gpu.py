"""avsd_ff_block (csrc/ffblock.hip, -m gpu): the tail of a 320-channel transformer block — LayerNorm-folded GEGLU projection, FF-out + h
and proj_out + x — as one launch, in both one-pass libraries; stage 1 alone (out = h') and stages 1 + 2.

Each case compares the fused output with (a) the three ops.gemm launches it replaces and (b) a float64 evaluation of LayerNorm, GEGLU,
FF-out + h, proj_out + x on the values the kernels read (the packed 16-bit weights) that rounds g and h' to the storage type where the
kernels do.  The bound has no constant of its own: rel_l2(fused, ref) <= 1.25 x rel_l2(separate, ref), the project's bound for a fused
launch (tests/test_qattn_gpu.py); here the margin covers f32 summation order only.

The kernel keeps every product's K order ascending, in 16-wide steps into one accumulator, and adds the epilogue terms in the shared
epilogue's order, so it is also held to bit identity with the three launches on the LDS-direct tile 9 with the unrotated K walk."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_l2
from tests.test_blocks_gpu import prec  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)]

C, HID, MMAX = 320, 1280, 384
EPS = 1e-5


@pytest.fixture
def ops(prec):
    from asva_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


_CACHE: dict = {}


def operands(ops, prec):
    """384 rows of operands per precision, built once and never written again: smaller cases take the first M rows"""
    if prec in _CACHE:
        return _CACHE[prec]
    from types import SimpleNamespace

    from asva_amd import precision as P
    from asva_amd.weights import pack_frag, pack_geglu, to_act

    def rndf(*shape, seed=0, scale=1.0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dev())

    o = SimpleNamespace()
    a0 = to_act(rndf(MMAX, C, seed=1))
    w0 = to_act(rndf(C, C, seed=2, scale=C ** -0.5))
    res0 = to_act(rndf(MMAX, C, seed=3) + 0.5)
    o.stats = torch.empty(MMAX, C // 32, 2, device=dev())
    o.h = ops.gemm(a0, w0, res1=res0, rowstats=o.stats)                     # residual stream + its LayerNorm statistics
    gamma, beta = 1 + 0.1 * rndf(C, seed=4), 0.1 * rndf(C, seed=5)
    w1, b1 = rndf(2 * HID, C, seed=6, scale=C ** -0.5), 0.1 * rndf(2 * HID, seed=7)
    o.w1_ln, o.b1_ln = pack_geglu(w1 * gamma[None, :], w1 @ beta + b1)       # as Packer.tr (asva_amd/unet.py)
    o.s1_ln = o.w1_ln.float().sum(1)
    o.w1_f = pack_frag(o.w1_ln)
    o.w2, o.b2 = to_act(rndf(C, HID, seed=8, scale=HID ** -0.5)), 0.1 * rndf(C, seed=9)
    o.wp, o.bp = to_act(rndf(C, C, seed=10, scale=C ** -0.5)), 0.1 * rndf(C, seed=11)
    o.w2_f, o.wp_f = pack_frag(o.w2), pack_frag(o.wp)
    o.x = to_act(rndf(MMAX, C, seed=12))
    # float64 on the same values, g and h' rounded to the storage type where the kernels round them
    hv = o.h.double()
    ln = (hv - hv.mean(1, keepdim=True)) * torch.rsqrt(hv.var(1, unbiased=False, keepdim=True) + EPS)
    y = (ln @ o.w1_ln.double().T + o.b1_ln.double()).reshape(MMAX, HID // 16, 2, 16)      # packed rows: [16 values | 16 gates] per block
    g = (y[:, :, 0] * F.gelu(y[:, :, 1])).reshape(MMAX, HID)
    o.ref_h2 = g.to(P.ACT).double() @ o.w2.double().T + o.b2.double() + hv
    o.ref_out = o.ref_h2.to(P.ACT).double() @ o.wp.double().T + o.bp.double() + o.x.double()
    torch.cuda.synchronize()
    _CACHE[prec] = o
    return o


def fused(ops, o, M, proj, h=None, x=None, out=None):
    h = o.h[:M] if h is None else h
    if not proj:
        return ops.ff_block(h, o.stats[:M], o.w1_f, o.s1_ln, o.b1_ln, o.w2_f, o.b2, out=out)
    return ops.ff_block(h, o.stats[:M], o.w1_f, o.s1_ln, o.b1_ln, o.w2_f, o.b2, o.wp_f, o.bp, o.x[:M] if x is None else x, out=out)


def separate(ops, o, M, proj, tile=0):
    """the launches of unet._transformer step 5"""
    g = ops.gemm(o.h[:M], o.w1_ln, bias=o.b1_ln, geglu=True, ln=(o.stats[:M], o.s1_ln, EPS), tile=tile, **({} if tile else {"w_frag": o.w1_f}))
    h2 = ops.gemm(g, o.w2, bias=o.b2, res1=o.h[:M], tile=tile)
    return ops.gemm(h2, o.wp, bias=o.bp, res1=o.x[:M], tile=tile) if proj else h2


# an exact band, one row into a second band, a partial last band, four bands
@pytest.mark.parametrize("proj", [False, True], ids=["stage1", "stage1+2"])
@pytest.mark.parametrize("M", [96, 97, 200, 384])
def test_ff_block_matches_separate_launches_and_float64(ops, prec, M, proj):
    from asva_amd import precision as P

    o = operands(ops, prec)
    out = fused(ops, o, M, proj)
    assert out.dtype == P.ACT and out.shape == (M, C)
    sep = separate(ops, o, M, proj)
    ref = (o.ref_out if proj else o.ref_h2)[:M]
    e_fused, e_sep = rel_l2(out, ref), rel_l2(sep, ref)
    print(f"ff_block {prec} M={M} proj_out={proj}: fused vs float64 {e_fused:.4e}, separate vs float64 {e_sep:.4e}, "
          f"fused vs separate {rel_l2(out, sep):.4e}")
    assert e_fused <= 1.25 * e_sep, (e_fused, e_sep)
    # a repeat run is bit-identical
    assert torch.equal(fused(ops, o, M, proj), out)
    # K ascending in every product: bit-identical to the three launches on the LDS-direct tile 9, unrotated
    ops.set_krot(False)
    try:
        want = separate(ops, o, M, proj, tile=9)
    finally:
        ops.set_krot(True)
    assert torch.equal(out, want)


@pytest.mark.parametrize("proj", [False, True], ids=["stage1", "stage1+2"])
@pytest.mark.parametrize("M", [97, 200])
def test_ff_block_padding_and_strides(ops, prec, M, proj):
    """h, x and out as column slices of wider buffers (ld = C + 16) with rows past M: the rows of h and x past M hold 3e4 and never reach
    the result, columns outside C and rows past M of the output buffer keep their sentinel"""
    from asva_amd import precision as P

    o = operands(ops, prec)
    want = fused(ops, o, M, proj)
    rows = (M + 95) // 96 * 96 + 8
    hb = torch.full((rows, C + 16), 3.0e4, dtype=P.ACT, device=dev())
    xb = torch.full((rows, C + 16), 3.0e4, dtype=P.ACT, device=dev())
    hb[:M, 8:8 + C], xb[:M, 8:8 + C] = o.h[:M], o.x[:M]
    ob = torch.full((rows, C + 16), 7.0, dtype=P.ACT, device=dev())
    got = fused(ops, o, M, proj, h=hb[:M, 8:8 + C], x=xb[:M, 8:8 + C], out=ob[:M, 8:8 + C])
    assert torch.equal(got, want)
    assert bool((ob[:, :8] == 7.0).all()) and bool((ob[:, 8 + C:] == 7.0).all()) and bool((ob[M:] == 7.0).all())


def test_ff_block_refuses_what_is_not_built(ops, prec):
    from asva_amd import _lib
    from asva_amd import precision as P

    o = operands(ops, prec)

    def refused(call, out):
        with pytest.raises(_lib.AvsdError, match=r"avsd_ff_block failed \(code -1\): ff_block: unsupported"):
            call(out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())          # AVSD_EINVAL: nothing was launched

    # C = 640
    M, C2 = 96, 640
    z16 = lambda *s: torch.zeros(*s, dtype=P.ACT, device=dev())         # noqa: E731
    z32 = lambda *s: torch.zeros(*s, device=dev())                      # noqa: E731
    assert not ops.ff_block_supported(24576, C2, True) and not ops.ff_block_supported(24576, C2, False)
    refused(lambda out: ops.ff_block(z16(M, C2), z32(M, C2 // 32, 2), z16(8 * C2 // 32, C2 // 16, 64, 8), z32(8 * C2), z32(8 * C2),
                                     z16(C2 // 32, 4 * C2 // 16, 64, 8), z32(C2), z16(C2 // 32, C2 // 16, 64, 8), z32(C2), z16(M, C2), out=out),
            torch.full((M, C2), 7.0, dtype=P.ACT, device=dev()))
    # ld = C + 4
    hb = z16(M, C + 4)
    hb[:, :C] = o.h[:M]
    refused(lambda out: fused(ops, o, M, True, h=hb[:, :C], out=out), torch.full((M, C), 7.0, dtype=P.ACT, device=dev()))
    ob = torch.full((M, C + 4), 7.0, dtype=P.ACT, device=dev())
    refused(lambda out: fused(ops, o, M, False, out=out[:, :C]), ob)
    # M = 0
    assert not ops.ff_block_supported(0, C, True)
    refused(lambda out: fused(ops, o, 0, True, out=out[:0]), torch.full((8, C), 7.0, dtype=P.ACT, device=dev()))


def _block(M_, prec_name, fuse_ff, B, Fr, H, W, text, audio, x):
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
    old = unet._FUSE_FF
    unet._FUSE_FF = fuse_ff
    try:
        out = M_._transformer(st, _Act(_ops.to_act(x)), root.p, (H, W), 8)
    finally:
        unet._FUSE_FF = old
    return _ops.from_act(out.lo).float()


def test_transformer_block_with_and_without_the_fused_tail(ops, prec):
    """unet._transformer at C = 320 on the smallest geometry ops.ff_block_supported admits, hook on and off.  The reference is the same block
    in split precision (16 significant bits in every stored value), which tests/test_blocks_gpu.py holds to < 2e-5 of the reference
    implementation's fp32 module — two orders below the errors compared here."""
    from asva_amd import precision as P
    from asva_amd.unet import AudioUNet3DConditionModel as M_
    from oracle.filler import seeded_randn_bf16

    geo = next(((B, Fr, H, W) for B, Fr, H, W in [(1, 4, 48, 64), (1, 8, 48, 64), (2, 8, 48, 64)] if ops.ff_block_supported(B * Fr * H * W, C, True)), None)
    assert geo is not None, "ff_block_supported admits none of the block-test geometries"
    B, Fr, H, W = geo
    x = seeded_randn_bf16(101, B, C, Fr, H, W).permute(0, 2, 3, 4, 1).reshape(-1, C).cuda().contiguous()
    text, audio = seeded_randn_bf16(102, B, 77, 768).cuda(), seeded_randn_bf16(103, B, 229, 768).cuda()
    try:
        ref = _block(M_, "bf16x2", False, B, Fr, H, W, text, audio, x)
        on = _block(M_, prec, True, B, Fr, H, W, text, audio, x)
        off = _block(M_, prec, False, B, Fr, H, W, text, audio, x)
    finally:
        P.set_split(False)
        P.set_precision(prec)
    e_on, e_off = rel_l2(on, ref), rel_l2(off, ref)
    print(f"transformer block {prec} M={B * Fr * H * W}: fused tail vs split precision {e_on:.4e}, three launches {e_off:.4e}, "
          f"fused vs three launches {rel_l2(on, off):.4e}")
    assert e_on <= 1.25 * e_off, (e_on, e_off)
