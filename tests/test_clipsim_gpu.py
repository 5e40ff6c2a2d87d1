"""CLIPSim / AlignSync on the MI355X (asva_amd/imagebind_eval.py, csrc/imagebind_eval.hip), in both builds of the library.

Truth is float64 (torch on the CPU; for the towers the restatement tests/imagebind_ref.py, which tests/test_clipsim_cpu.py pins to
transformers; its outputs are the fixtures tests/golden/clipsim/, written by tools/gen_clipsim_golden.py).  Tolerance rule for every
f32 kernel, as tests/test_clip_text_gpu.py: e_ref = rel-L2 error against float64 of torch's fp32 CPU result for the same input; the
kernel's rel-L2 error against float64 must stay within 4 x e_ref.  No bound comes from what the kernels give.  Each test prints
`MEASURED <name> e_ref=<..> kernel=<..>` (run with -s).  A library that is not built is a failure, not a skip.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import imagebind_ref as R
from tests.helpers import GOLDEN, load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIR = os.path.join(GOLDEN, "clipsim")


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """the library the test runs in; a library that is not built is a build failure, not missing hardware"""
    from asva_amd import _lib, precision

    assert os.path.isfile(_lib.LIB_PATHS[request.param]), f"the {request.param} library is not built"
    precision.set_precision(request.param)
    yield request.param
    precision.set_precision("bf16")


def _in_build(name, fn):
    from asva_amd import _lib, precision

    assert os.path.isfile(_lib.LIB_PATHS[name]), f"the {name} library is not built"
    precision.set_precision(name)
    try:
        return fn()
    finally:
        precision.set_precision("bf16")


def _within(name, got, ref32, ref64, factor=4.0):
    e_ref, e_k = R.rel_l2(ref32, ref64), R.rel_l2(got, ref64)
    print(f"MEASURED {name} e_ref={e_ref:.4e} kernel={e_k:.4e}")
    assert e_k <= factor * e_ref, (name, e_k, e_ref)
    return e_ref, e_k


_CASES = {}


def _case(name):
    """(config, seeded state dict, seeded inputs, fixture, CLIPModel on the device), built once"""
    from asva_amd.imagebind_eval import CLIPModel

    if name not in _CASES:
        config = R.CONFIGS[name]
        sd = R.draw_state_dict(config)
        g = torch.load(os.path.join(DIR, name + ".pt"), map_location="cpu", weights_only=True)
        for k, probe in g["probe"].items():
            assert torch.equal(sd[k].flatten()[:4], probe), f"the seeded draw of {k} no longer matches the fixture"
        m = CLIPModel(config)
        m.load_state_dict(sd)
        _CASES[name] = (config, sd, R.make_inputs(name), g, m.to(DEV))
    return _CASES[name]


# ---- avsd_attention_f32 ------------------------------------------------------------------------------------------------------------------
ATTN = [(257, 80), (230, 64), (33, 80), (32, 64), (1, 64)]
HEADS = 2
_ATTN_REF = {}


def _attn_buf(b, seq, d):
    """one [b * seq, 3 C + 64] buffer: q | k | v and 64 surplus columns of NaN.  Row 1 of every sequence has scores near +80, row 2 (or the
    last row) near -80: k carries a shared component of ones, so a constant query c * ones scores c * scale * (d + sum k_j)"""
    c = HEADS * d
    g = torch.Generator().manual_seed(1000 * seq + d)
    buf = torch.randn(b * seq, 3 * c + 64, generator=g)
    buf[:, :c] *= 1.5                                             # a peaked softmax
    buf[:, c:2 * c] += 1.0
    q = buf.view(b, seq, -1)[:, :, :c]
    q[:, min(1, seq - 1)] = 80.0 / (d ** 0.5)                     # scale * (80 / sqrt d) * (d + sum k_j) = 80 (1 + mean k_j)
    q[:, min(2, seq - 1)] = -80.0 / (d ** 0.5)
    buf[:, 3 * c:] = float("nan")
    return buf


def _attn_ref(buf, b, seq, d, dtype):
    key = (b, seq, d, dtype)
    if key not in _ATTN_REF:
        c = HEADS * d
        q, k, v = (buf[:, i * c:(i + 1) * c].to(dtype).view(b, seq, HEADS, d).transpose(1, 2) for i in range(3))
        _ATTN_REF[key] = F.scaled_dot_product_attention(q, k, v, scale=d ** -0.5).transpose(1, 2).reshape(b * seq, c)
    return _ATTN_REF[key]


def _attn(buf, b, seq, d):
    from asva_amd import ops

    c = HEADS * d
    return ops.attention_f32(buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:3 * c], b, seq, HEADS)


@pytest.mark.parametrize("seq,d", ATTN)
def test_attention_against_float64_sdpa(build, seq, d):
    b, c = 2, HEADS * d
    buf = _attn_buf(b, seq, d)
    dev = buf.to(DEV)
    out = _attn(dev, b, seq, d)
    assert out.shape == (b * seq, c) and bool(torch.isfinite(out).all())
    back = dev.cpu()
    assert torch.equal(back[:, :3 * c], buf[:, :3 * c]) and bool(torch.isnan(back[:, 3 * c:]).all())       # the buffer is untouched
    if seq == 1:                                                  # one key: the output is V itself
        assert torch.equal(out.cpu(), buf[:, 2 * c:3 * c])
        return
    _within(f"attention_f32_L{seq}_d{d}", out, _attn_ref(buf, b, seq, d, torch.float32), _attn_ref(buf, b, seq, d, torch.float64))
    rows = [s * seq + r for s in range(b) for r in (min(1, seq - 1), min(2, seq - 1))]                       # the +-80 rows on their own
    _within(f"attention_f32_L{seq}_d{d}_rows80", out[rows], _attn_ref(buf, b, seq, d, torch.float32)[rows],
            _attn_ref(buf, b, seq, d, torch.float64)[rows])


@pytest.mark.parametrize("seq,d", ATTN)
def test_attention_is_batch_invariant_and_deterministic(build, seq, d):
    buf = _attn_buf(3, seq, d).to(DEV)
    full = _attn(buf, 3, seq, d)
    assert torch.equal(full, _attn(buf, 3, seq, d))
    assert torch.equal(_attn(buf[seq:2 * seq], 1, seq, d), full[seq:2 * seq])


@pytest.mark.parametrize("seq,d", ATTN)
def test_attention_gives_the_same_bits_in_both_builds(seq, d):
    buf = _attn_buf(2, seq, d).to(DEV)
    a, b = (_in_build(name, lambda: _attn(buf, 2, seq, d).clone()) for name in ("bf16", "fp16"))
    assert torch.equal(a, b)


def test_attention_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    buf = torch.zeros(4, 3 * 96, device=DEV)
    with pytest.raises(_lib.AvsdError, match="head dims 64 and 80"):
        ops.attention_f32(buf[:, :96], buf[:, 96:192], buf[:, 192:], 1, 4, 2)
    with pytest.raises(ValueError, match="heads \\* d"):
        ops.attention_f32(buf[:, :96], buf[:, 96:192], buf[:3, 192:], 1, 4, 2)


# ---- pointwise and row kernels ----------------------------------------------------------------------------------------------------------
def test_gelu_in_place_with_extreme_values(build):
    from asva_amd import ops

    n = 257 * 256 + 3
    x = 3.0 * torch.randn(n, generator=torch.Generator().manual_seed(3))
    x[:8] = torch.tensor([100.0, -100.0, 1e4, -1e4, 0.0, -0.0, 6.0, -6.0])
    ref32, ref64 = F.gelu(x), F.gelu(x.double())
    xd = x.to(DEV)
    out = ops.gelu_f32(xd, out=xd)
    assert out.data_ptr() == xd.data_ptr() and bool(torch.isfinite(out).all())
    _within("gelu", out, ref32, ref64)
    assert out[:6].cpu().tolist() == [100.0, 0.0, 1e4, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("tail", [0, 1])
def test_vit_tokens_is_exact(build, tail):
    from asva_amd import ops

    g = torch.Generator().manual_seed(4)
    b, n, c = 3, 16, 160
    patches, cls, pos = torch.randn(b * n, c, generator=g), torch.randn(c, generator=g), torch.randn(1 + n, c, generator=g)
    out = ops.vit_tokens_f32(patches.to(DEV), cls.to(DEV), pos.to(DEV), b, tail_rows=tail).cpu().view(b, 1 + n + tail, c)
    assert torch.equal(out[:, 0], (cls + pos[0]).expand(b, c)) and torch.equal(out[:, 1:1 + n], patches.view(b, n, c) + pos[1:])
    assert tail == 0 or torch.equal(out[:, 1 + n:], torch.zeros(b, tail, c))


@pytest.mark.parametrize("c", [1024, 100])
@pytest.mark.parametrize("rep", [1, 12])
def test_cosine_rows_against_float64(build, c, rep):
    from asva_amd import ops

    g = torch.Generator().manual_seed(c + rep)
    m = 2 * rep + (0 if rep > 1 else 3)
    x, y = torch.randn(m, c, generator=g), torch.randn(m // rep, c, generator=g) * 3.0
    x[1] = 0.0                                                    # a zero row gives 0, not NaN
    yy = y.repeat_interleave(rep, dim=0)
    out = ops.cosine_rows_f32(x.to(DEV), y.to(DEV), rep)
    assert out.shape == (m,) and bool(torch.isfinite(out).all()) and float(out[1]) == 0.0
    _within(f"cosine_rows_c{c}_rep{rep}", out, R.cosine(x, yy), R.cosine(x.double(), yy.double()))
    # a row's result does not depend on where it sits or on rep
    assert torch.equal(ops.cosine_rows_f32(x[:1].to(DEV), y[:1].to(DEV), 1), out[:1])
    nrm = ops.normalize_rows_f32(x.to(DEV))
    _within(f"normalize_rows_c{c}", nrm, F.normalize(x, dim=-1), F.normalize(x.double(), dim=-1))
    assert bool((nrm[1] == 0).all())


# ---- towers with seeded weights against the restatement in float64 ---------------------------------------------------------------------------
def _encode(name):
    _, _, x, _, m = _case(name)
    if "images" in x:
        return m.encode_image(x["images"].to(DEV))
    if "ids" in x:
        return m.encode_text(x["ids"])
    return m.encode_audio(x["audios"].to(DEV))


@pytest.mark.parametrize("name", ["v80", "v64", "vh1", "t64", "a1"])
def test_tower_against_the_float64_restatement(build, name):
    g = _case(name)[3]
    out = _encode(name)
    assert out.shape == g["ref64"].shape and out.dtype == torch.float32
    assert float((out.double().norm(dim=-1) - 1.0).abs().max()) <= 1e-6          # unit norm
    _within(f"tower_{name}", out, g["ref32"], g["ref64"])


@pytest.mark.parametrize("name", ["v80", "t64", "a1"])
def test_towers_give_the_same_bits_in_both_builds_and_any_batch(name):
    a, b = (_in_build(bld, lambda: _encode(name).clone()) for bld in ("bf16", "fp16"))
    assert torch.equal(a, b)
    _, _, x, _, m = _case(name)
    if "images" in x:
        alone = m.encode_image(x["images"][1:].to(DEV))
    elif "ids" in x:
        alone = m.encode_text(x["ids"][1:2])
    else:
        alone = m.encode_audio(x["audios"][1:].to(DEV))
    assert torch.equal(alone[0], a[1])


# ---- metric level (tiny towers) ------------------------------------------------------------------------------------------------------------------
def test_clip_consistency_against_restatement_and_direct_call(build):
    from asva_amd.imagebind_eval import compute_clip_consistency, preprocess_videos

    _, _, x, g, m = _case("tiny")
    videos, audios, ids = x["videos"].to(DEV), x["audios"].to(DEV), x["ids"]
    out = compute_clip_consistency(videos, audios, ids, net=m)
    assert sorted(out) == ["ia_sim", "it_sim"] and all(v.shape == (2, 3) and v.dtype == torch.float32 for v in out.values())
    for k in out:
        _within(f"clip_consistency_{k}", out[k], g["ref32"][k], g["ref64"][k])
    # the reference's way: frame-repeated audios and texts through net(...)
    frames, rep_a, rep_t = preprocess_videos(videos, audios, ids, size=56)
    assert frames.shape == (6, 3, 56, 56) and rep_a.shape == (6, 1, 128, 204) and rep_t.shape == (6, 77)
    direct = m(frames, rep_a, rep_t)
    assert torch.equal(direct["ia_sim"].view(2, 3), out["ia_sim"]) and torch.equal(direct["it_sim"].view(2, 3), out["it_sim"])
    only = compute_clip_consistency(videos, audios, net=m)
    assert sorted(only) == ["ia_sim"] and torch.equal(only["ia_sim"], out["ia_sim"])


def test_alignsync_with_the_seeded_classifier(build):
    from asva_amd import avsync as A
    from asva_amd.imagebind_eval import alignsync_from_sims, compute_alignsync, compute_clip_consistency
    from tests import avsync_ref as AR

    m = _case("tiny")[4]
    fx = load_golden("avsync_tiny.pt")
    net = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    net.load_state_dict(AR.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), fx["seed"]))
    net = net.to(DEV)
    t = torch.arange(32000, dtype=torch.float32) / 16000.0
    wave = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) * (1.0 + torch.sin(2 * torch.pi * 3.0 * t)))[None]
    clip = AR.u8_to_unit(AR.grating_video_u8(12, 64, 64, 0.7, 0.13, 23.0))                                 # (3, 12, 64, 64)
    ref = AR.u8_to_unit(AR.grating_video_u8(12, 64, 64, 2.2, -0.3, 41.0, mean=0.4, contrast=0.3))
    got = A.compute_sync_metrics_on_av(wave, 16000, clip, ref_video=ref, metric="alignsync", net=net, clip_net=m)
    assert got.shape == () and 0.0 < float(got) < 1.0
    from asva_amd.audio_features import waveform_to_melspectrogram

    mel = waveform_to_melspectrogram(wave, device=DEV)[None].contiguous()
    v, r = clip[None].to(DEV), ref[None].to(DEV)
    assert torch.equal(got, compute_alignsync(mel, v, r, net, m)[0])
    # composed by hand: RelSync times the mean align probability of [reference frame 0, generated frames 1..]
    rel = A.compute_relsync(mel, v, net, ref_videos=r)
    mixed = torch.cat([r[:, :, :1], v[:, :, 1:]], dim=2).permute(0, 2, 1, 3, 4)
    ia = compute_clip_consistency(mixed, mel, net=m)["ia_sim"].cpu()
    assert ia.shape == (1, 12) and torch.equal(got, alignsync_from_sims(ia, rel)[0])
    want = torch.sigmoid(ia[0, 1:].double() - ia[0, 0].double()).mean() * rel[0].double()
    assert abs(float(got) - float(want)) <= 1e-6
