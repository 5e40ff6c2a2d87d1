"""avsd_qproj_attention (csrc/qattn.hip, -m gpu): the LayerNorm-folded Q projection and the cross-attention over cached, padded K / V^T as
one launch, at the widths the one-launch block (xattn.hip) is not built for — C = 640 (8 heads of 80) and C = 1280 (8 heads of 160) — in
both one-pass libraries.

Each case compares the fused output with (a) the two launches it replaces and (b) an fp32 LayerNorm + scaled_dot_product_attention.  The
bound has no constant of its own: rel_l2(fused, fp32) <= 1.25 x rel_l2(separate, fp32), the error of the path it replaces on the same
operands; the margin is for the different f32 summation order and for q no longer being rounded to 16 bits between the launches."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_l2, xattn_block_operands
from tests.test_blocks_gpu import prec  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)]


@pytest.fixture
def ops(prec):
    from asva_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


def fused(ops, p, k_pad=None, vt_pad=None, out=None):
    return ops.qproj_attention(p.h, p.stats, p.wq_f, p.q_colsum, p.q_bias, p.k_pad if k_pad is None else k_pad,
                               p.vt_pad if vt_pad is None else vt_pad, p.lk, heads=p.heads, L=p.L, q_per_kv=p.q_per_kv, out=out)


# (kind, keys, K/V per frame, B, frames, rows per frame): M = 384 rows everywhere
CASES = [
    ("text", 77, False, 2, 3, 64),            # keys shared by the frames of a clip: 192 rows per K/V block
    ("audio", 25, True, 2, 3, 64),            # gathered per frame: one 64-row tile per K/V block
    ("one_past_tile", 33, True, 2, 3, 64),    # one key past a 32-key tile
    ("no_padding", 96, False, 2, 3, 64),
    ("text_4x4", 77, False, 2, 12, 16),       # a row tile spans four frames of one clip (12 frames as in the UNet: 192 rows per K/V block;
                                              # with 3 frames a block has 48 rows, which is no whole row tile and therefore not built)
    ("audio_128", 25, True, 1, 3, 128),       # 128 rows per K/V block: the 128-row tile at C = 640
]


@pytest.mark.parametrize("C", [640, 1280])
@pytest.mark.parametrize("kind,lk,per_frame,B,Fr,L", CASES, ids=[c[0] for c in CASES])
def test_qproj_attention_matches_separate_kernels_and_fp32(ops, prec, C, kind, lk, per_frame, B, Fr, L):
    from asva_amd import precision as P

    p = xattn_block_operands(ops, P.ACT, lk, per_frame, False, B=B, Fr=Fr, L=L, C=C, heads=8)
    heads, d, M, nkv = p.heads, p.d, p.M, p.nkv
    assert M == 384 and ops.qproj_attention_supported(C, heads, p.k_pad.shape[1], M, L, p.q_per_kv)
    out = fused(ops, p)
    assert out.dtype == P.ACT and out.shape == (M, C)
    # (a) the two launches it replaces
    q = ops.gemm(p.h, p.wq_f, bias=p.q_bias, ln=(p.stats, p.q_colsum, 1e-5))
    sep = ops.attention(q, p.kk.reshape(nkv * lk, C), p.vv.reshape(nkv * lk, C), bq=B * Fr, lq=L, lk=lk, kv_rows=lk, heads=heads,
                        q_per_kv=p.q_per_kv, frames=Fr)
    # (b) fp32
    hn = F.layer_norm(p.h.float(), (C,), p.gamma, p.beta, 1e-5)
    qf = (hn @ p.wq.T).reshape(B * Fr, L, heads, d).transpose(1, 2)
    kv_of = torch.arange(B * Fr, device=dev()) // p.q_per_kv
    kf = p.kk.float()[kv_of].reshape(B * Fr, lk, heads, d).transpose(1, 2)
    vf = p.vv.float()[kv_of].reshape(B * Fr, lk, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(M, C)
    e_fused, e_sep = rel_l2(out, ref), rel_l2(sep, ref)
    print(f"qproj_attention {prec} C={C} {kind} lk={lk}: fused vs fp32 {e_fused:.4e}, separate vs fp32 {e_sep:.4e}, "
          f"fused vs separate {rel_l2(out, sep):.4e}")
    assert e_fused <= 1.25 * e_sep, (e_fused, e_sep)
    # bit-repeatable
    assert torch.equal(fused(ops, p), out)
    # the padding is never read into the result: key rows lk .. lk_pad of K and the matching columns of V^T refilled with large finite values
    if p.k_pad.shape[1] > lk:
        k2, vt2 = p.k_pad.clone(), p.vt_pad.clone()
        k2[:, lk:] = 3.0e4
        vt2[:, :, lk:] = -3.0e4
        assert torch.equal(fused(ops, p, k2, vt2), out)
    # an output that is a column slice of a wider buffer (ldo > C) is written inside its columns only
    buf = torch.zeros(M, C + 16, dtype=P.ACT, device=dev())
    assert torch.equal(fused(ops, p, out=buf[:, 8:8 + C]), out) and not buf[:, :8].any() and not buf[:, 8 + C:].any()


def test_qproj_attention_refuses_what_is_not_built(ops, prec):
    from asva_amd import _lib
    from asva_amd import precision as P

    def refused(p, k_pad=None, vt_pad=None):
        out = torch.full((p.M, p.C), 7.0, dtype=P.ACT, device=dev())
        with pytest.raises(_lib.AvsdError, match=r"avsd_qproj_attention failed \(code -1\): qproj_attention: unsupported shape"):
            fused(ops, p, k_pad, vt_pad, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())          # AVSD_EINVAL: nothing was launched

    # audio at 4 x 4: 16 rows per K/V block, less than a row tile
    p = xattn_block_operands(ops, P.ACT, 25, True, False, B=2, Fr=12, L=16, C=640, heads=8)
    assert not ops.qproj_attention_supported(640, 8, 32, p.M, 16, 1)
    refused(p)
    p = xattn_block_operands(ops, P.ACT, 25, True, False, B=2, Fr=12, L=16, C=1280, heads=8)
    assert not ops.qproj_attention_supported(1280, 8, 32, p.M, 16, 1)
    refused(p)
    # lk_pad = 128
    p = xattn_block_operands(ops, P.ACT, 77, False, False, B=2, Fr=3, L=64, C=640, heads=8)
    assert ops.qproj_attention_supported(640, 8, 96, p.M, 64, 3) and not ops.qproj_attention_supported(640, 8, 128, p.M, 64, 3)
    k128 = torch.zeros(p.nkv, 128, 640, dtype=P.ACT, device=dev())
    vt128 = torch.zeros(p.nkv, 640, 128, dtype=P.ACT, device=dev())
    k128[:, :96], vt128[:, :, :96] = p.k_pad, p.vt_pad
    refused(p, k128, vt128)
    # C = 320: the one-launch block's width
    p = xattn_block_operands(ops, P.ACT, 77, False, False, B=2, Fr=3, L=64, C=320, heads=8)
    assert not ops.qproj_attention_supported(320, 8, 96, p.M, 64, 3)
    refused(p)
