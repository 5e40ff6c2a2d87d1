"""AVSync scorer on the MI355X (asva_amd/avsync.py, csrc/avsync.hip), in both builds of the library.

Bounds (none comes from what the kernels give):
  * one product on v_mfma_f32_32x32x2_f32 against float64: rel-L2 < 1e-6, the bound tests/test_split_gpu.py::
    test_f32_yardstick_gemm_is_exact_f32 uses for the same instruction (measured 1 - 5e-7 there);
  * whole classifier: about twenty products in series, each inside 5e-7, ReLU and mean do not amplify: 20 x 5e-7 = 1e-5 is the linear
    worst case -> embeddings rel-L2 < 1e-5, scores within 1e-5 (1 + |s|), RelSync within 1e-5;
  * max-pool exact; row mean < 1e-6; resize + normalise: the bound of the CPU test (tests/golden/avsync_measured.json, below 1e-5).
Measured on MI355X: tests/golden/avsync_measured.json, "gpu".
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import avsync_ref as R
from tests.helpers import GOLDEN, ROOT, load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """the library the test runs in; only a library that is not built may skip"""
    from asva_amd import _lib, precision

    if not os.path.isfile(_lib.LIB_PATHS[request.param]):
        pytest.skip(f"the {request.param} library is not built")
    precision.set_precision(request.param)
    yield request.param
    precision.set_precision("bf16")


def _in_build(name, fn):
    from asva_amd import precision

    precision.set_precision(name)
    try:
        return fn()
    finally:
        precision.set_precision("bf16")


def _both_built():
    from asva_amd import _lib

    if not all(os.path.isfile(p) for p in _lib.LIB_PATHS.values()):
        pytest.skip("needs both the bf16 and the fp16 library")


@pytest.fixture(scope="module")
def fixture():
    g = load_golden("avsync_tiny.pt")
    sd = R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    g["video"] = R.normalize_clip(R.u8_to_unit(g["video_u8"]))
    return g


@pytest.fixture(scope="module")
def net(fixture):
    from asva_amd import avsync as A

    m = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    m.load_state_dict(fixture["sd"])
    return m.to(DEV)


# ---- avsd_convnd_f32 ---------------------------------------------------------------------------------------------------------------
# (name, taps, stride, pad, cin, cout, (n, t, h, w)): the seven layer shapes of the two networks, then odd sizes
CONV_CASES = [
    ("stem_3x7x7_s122_cin3", (3, 7, 7), (1, 2, 2), (1, 3, 3), 3, 64, (1, 4, 30, 34)),
    ("spatial_1x3x3_s1", (1, 3, 3), (1, 1, 1), (0, 1, 1), 64, 64, (2, 3, 14, 12)),
    ("spatial_1x3x3_s122", (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 128, (2, 3, 14, 12)),
    ("temporal_3x1x1_s1", (3, 1, 1), (1, 1, 1), (1, 0, 0), 128, 128, (2, 6, 7, 6)),
    ("temporal_3x1x1_s211", (3, 1, 1), (2, 1, 1), (1, 0, 0), 128, 128, (2, 6, 7, 6)),
    ("projection_1x1x1_s222", (1, 1, 1), (2, 2, 2), (0, 0, 0), 64, 128, (2, 6, 14, 12)),
    ("audio_7x7_s2_cin1", (1, 7, 7), (1, 2, 2), (0, 3, 3), 1, 64, (2, 1, 128, 204)),
    ("audio_3x3_s1", (1, 3, 3), (1, 1, 1), (0, 1, 1), 256, 512, (2, 1, 16, 26)),
    ("audio_3x3_s2", (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 64, (2, 1, 64, 102)),
    # sizes not divisible by the stride, M not a multiple of any tile, cout 96 (an N tail), a large M (the 128-row tiles)
    ("odd_stem", (3, 7, 7), (1, 2, 2), (1, 3, 3), 3, 64, (1, 5, 33, 27)),
    ("odd_spatial_s122_cout96", (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 96, (1, 5, 13, 9)),
    ("odd_temporal_s211_cout96", (3, 1, 1), (2, 1, 1), (1, 0, 0), 64, 96, (1, 5, 5, 7)),
    ("odd_projection_s222", (1, 1, 1), (2, 2, 2), (0, 0, 0), 64, 96, (1, 5, 13, 9)),
    ("odd_audio_cin1", (1, 7, 7), (1, 2, 2), (0, 3, 3), 1, 64, (1, 1, 37, 51)),
    ("big_m_cout64", (1, 3, 3), (1, 1, 1), (0, 1, 1), 64, 64, (2, 6, 57, 55)),
    ("big_m_cout128", (1, 3, 3), (1, 1, 1), (0, 1, 1), 64, 128, (3, 8, 57, 55)),
    ("big_m_cin3_cout96", (1, 3, 3), (1, 1, 1), (0, 1, 1), 3, 96, (2, 8, 64, 64)),
    ("fc_1024_to_512", (1, 1, 1), (1, 1, 1), (0, 0, 0), 1024, 512, (3, 1, 1, 1)),
    ("fc_256_to_1", (1, 1, 1), (1, 1, 1), (0, 0, 0), 256, 1, (3, 1, 1, 1)),
]
# (bias, residual, rscale, relu)
EPILOGUES = [(False, False, False, False), (True, False, False, True), (True, True, False, True), (True, True, True, True),
             (False, True, True, False)]


def _conv_case(case, seed=0):
    name, taps, stride, pad, cin, cout, (n, t, h, w) = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, t, h, w, generator=g)
    wt = torch.randn(cout, cin, *taps, generator=g) * (2.0 / (cin * taps[0] * taps[1] * taps[2])) ** 0.5
    y64 = F.conv3d(x.double(), wt.double(), None, stride, pad)
    k = cin * taps[0] * taps[1] * taps[2]
    wp = torch.zeros(cout, (k + 3) // 4 * 4)
    wp[:, :k] = wt.permute(0, 2, 3, 4, 1).reshape(cout, k)
    return x, wp, y64, dict(bias=torch.randn(cout, generator=g), res=torch.randn(y64.shape, generator=g), rscale=0.5 + torch.rand(cout, generator=g))


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_convnd_f32_against_float64(build, case):
    from asva_amd import ops

    _, taps, stride, pad, cin, cout, _ = case
    x, wp, y64, e = _conv_case(case)
    xd, wd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV), wp.to(DEV)
    for use_bias, use_res, use_rs, relu in EPILOGUES:
        ref = y64.clone()
        if use_bias:
            ref += e["bias"].double().view(1, -1, 1, 1, 1)
        if use_res:
            ref += (e["rscale"].double().view(1, -1, 1, 1, 1) if use_rs else 1.0) * e["res"].double()
        if relu:
            ref = ref.relu()
        out = ops.convnd_f32(xd, wd, taps, stride, pad, bias=e["bias"].to(DEV) if use_bias else None,
                             res=e["res"].permute(0, 2, 3, 4, 1).contiguous().to(DEV) if use_res else None,
                             rscale=e["rscale"].to(DEV) if use_rs else None, relu=relu)
        assert out.shape == tuple(ref.permute(0, 2, 3, 4, 1).shape)
        err = R.rel_l2(out.permute(0, 4, 1, 2, 3), ref)
        print(f"convnd_f32 {case[0]} [{build}] bias={use_bias} res={use_res} rscale={use_rs} relu={relu}: rel-L2 {err:.3e}")
        assert err < 1e-6, (case[0], use_bias, use_res, use_rs, relu, err)


def test_convnd_f32_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    x = torch.zeros(1, 4, 8, 8, 64, device=DEV)
    w = torch.zeros(64, 576, device=DEV)
    with pytest.raises(ValueError):
        ops.convnd_f32(x, w, (1, 9, 9), (1, 1, 1), (0, 0, 0))                     # window larger than the image
    with pytest.raises(_lib.AvsdError, match="ldw"):
        ops.convnd_f32(x, w[:, :572].contiguous(), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    with pytest.raises(ValueError):
        ops.convnd_f32(x, w, (1, 3, 3), (1, 1, 1), (0, 1, 1), res=torch.zeros(1, 4, 8, 8, 32, device=DEV))


def test_linear_f32_is_the_convnd_f32_call_it_wraps(build):
    """ops.linear_f32 (the linear layers of the FID, FVD, CLIPSim and CLIP text networks): bit for bit the (1, 1, 1)-window convnd_f32
    on m 1 x 1 x 1 images, without and with bias, and with a residual; and within the bound of test_convnd_f32_against_float64"""
    from asva_amd import ops

    m, k, n = 3, 20, 5
    g = torch.Generator().manual_seed(5)
    x, w, b, res = (torch.randn(s, generator=g).to(DEV) for s in ((m, k), (n, k), (n,), (m, n)))
    one, zero = (1, 1, 1), (0, 0, 0)
    for bias, r in ((None, None), (b, None), (b, res), (None, res)):
        out = ops.linear_f32(x, w, bias, r)
        direct = ops.convnd_f32(x.view(m, 1, 1, 1, k), w, one, one, zero, bias=bias, res=None if r is None else r.view(m, 1, 1, 1, n))
        assert out.shape == (m, n) and out.dtype == torch.float32 and torch.equal(out, direct.view(m, n))
        ref = x.double() @ w.double().t() + (0 if bias is None else bias.double()) + (0 if r is None else r.double())
        assert R.rel_l2(out, ref) < 1e-6, (bias is not None, r is not None)
    assert torch.equal(ops.linear_f32(x, w), ops.linear_f32(x, w, None, None))


# ---- pooling, mean, preprocessing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 16, 64), (1, 2, 15, 9, 64), (1, 1, 1, 1, 8)])
def test_maxpool_is_exact(build, shape):
    from asva_amd import ops

    x = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    ref = F.max_pool3d(x.permute(0, 4, 1, 2, 3), (1, 3, 3), (1, 2, 2), (0, 1, 1)).permute(0, 2, 3, 4, 1)
    assert torch.equal(ops.maxpool_hw_f32(x.to(DEV)).cpu(), ref)


@pytest.mark.parametrize("shape", [(2, 98, 512), (3, 416, 512), (1, 37632, 64), (2, 5, 100)])
def test_mean_rows(build, shape):
    from asva_amd import ops

    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)) + 0.5
    err = R.rel_l2(ops.mean_rows_f32(x.to(DEV)), x.double().mean(1))
    print(f"mean_rows_f32 {shape} [{build}]: rel-L2 {err:.3e}")
    assert err < 1e-6


def _resize_bound():
    with open(os.path.join(GOLDEN, "avsync_measured.json")) as f:
        m = json.load(f)
    return min(4.0 * m["cpu"]["resize_tables_max_abs"], 1e-5)


@pytest.mark.parametrize("name", ["avsync_preprocess.pt", "avsync_preprocess_128x256.pt"])
def test_resize_normalize_against_fixture(build, name):
    from asva_amd import avsync as A

    g = load_golden(name)
    frames = R.u8_to_unit(g["frames_u8"])                                   # (n, 3, H, W)
    out = A.preprocess_videos(frames.permute(1, 0, 2, 3)[None].to(DEV))      # (1, 3, n, 224, 224)
    assert out.shape == (1, 3, frames.shape[0], 224, 224)
    err = (out[0].permute(1, 0, 2, 3).cpu() - g["out"]).abs().max().item()
    print(f"resize_aa_normalize_f32 {name} [{build}]: max abs {err:.3e} (bound {_resize_bound():.3e})")
    assert err <= _resize_bound()


# ---- the whole classifier ----------------------------------------------------------------------------------------------------------------
def _check_scores(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    assert bool(((got - want).abs() <= 1e-5 * (1.0 + want.abs())).all()), (got, want)
    return ((got - want).abs() / (1.0 + want.abs())).max().item()


def test_classifier_against_fixture(build, net, fixture):
    from asva_amd import avsync as A

    audio, video = fixture["audio"].to(DEV), fixture["video"].to(DEV)
    a_st, v_st = [], []
    a, v = net.embed_audio(audio, stages=a_st), net.embed_video(video, stages=v_st)
    ea, ev = R.rel_l2(a, fixture["audio_emb"]), R.rel_l2(v, fixture["video_emb"])
    print(f"classifier vs fixture [{build}]: audio embedding rel-L2 {ea:.3e}, video embedding rel-L2 {ev:.3e}")
    # intermediate stage means of sample 0 (localises a wrong layer)
    for prefix, names, st in (("a.", ["conv1", "block1", "block2", "block3", "block4"], a_st), ("v.", ["conv1", "conv2x", "conv3x", "conv4x", "conv5x"], v_st)):
        for nm, y in zip(names, st):
            got = y[0].reshape(-1, y.shape[-1]).double().mean(0)
            e = R.rel_l2(got, fixture["stage_means"][prefix + nm])
            print(f"  stage {prefix}{nm}: rel-L2 of the position mean {e:.3e}")
            assert e < 1e-5, (prefix + nm, e)
    assert ea < 1e-5 and ev < 1e-5
    scores = torch.stack([torch.stack([net(audio[i:i + 1], video[j:j + 1])[0] for j in range(2)]) for i in range(2)])
    es = _check_scores(scores, fixture["scores"])
    own = torch.stack([scores[0, 0], scores[1, 1]])
    rs_a = A.relsync_from_scores(torch.stack([scores[1, 0], scores[0, 1]]), own)
    rs_v = A.relsync_from_scores(torch.stack([scores[0, 1], scores[1, 0]]), own)
    er = max((rs_a.cpu() - fixture["relsync_ref_audio"]).abs().max().item(), (rs_v.cpu() - fixture["relsync_ref_video"]).abs().max().item())
    print(f"  scores: max |d| / (1 + |s|) {es:.3e}; RelSync max |d| {er:.3e}")
    assert er <= 1e-5


@pytest.mark.parametrize("shape", [(1, 3, 12, 224, 224), (2, 3, 5, 96, 80)], ids=["1x12x224x224", "2x5x96x80"])
def test_classifier_against_restatement(build, net, fixture, shape):
    from asva_amd import avsync as A

    b = shape[0]
    g = torch.Generator().manual_seed(7)
    video_u8 = torch.stack([R.grating_video_u8(shape[2], shape[3], shape[4], 0.4 + 1.3 * i, 0.09 - 0.2 * i, 11.0 + 14.0 * i, 0.5 * i) for i in range(b)])
    video = R.normalize_clip(R.u8_to_unit(video_u8)) + 0.05 * torch.randn(shape, generator=g)
    audio = fixture["audio"][:b]
    sd = fixture["sd"]
    with torch.no_grad():
        a_ref = R.audio_forward(R._sub(sd, "audio_encoder."), audio)
        v_ref = R.video_forward(R._sub(sd, "video_encoder."), video)
        s_ref = R.head_forward(R._sub(sd, "head."), a_ref, v_ref)[:, 0]
        s_ref_swapped = R.head_forward(R._sub(sd, "head."), a_ref.flip(0), v_ref)[:, 0]
    a, v = net.embed_audio(audio.to(DEV)), net.embed_video(video.to(DEV))
    s = net(audio.to(DEV), video.to(DEV))
    s_swapped = net(audio.flip(0).to(DEV), video.to(DEV))
    ea, ev = R.rel_l2(a, a_ref), R.rel_l2(v, v_ref)
    es = max(_check_scores(s, s_ref), _check_scores(s_swapped, s_ref_swapped))
    er = (A.relsync_from_scores(s_swapped, s).cpu() - R.relsync(s_ref_swapped, s_ref)).abs().max().item()
    print(f"classifier vs restatement {shape} [{build}]: audio {ea:.3e}, video {ev:.3e}, scores {es:.3e}, RelSync {er:.3e}")
    assert ea < 1e-5 and ev < 1e-5 and er <= 1e-5


def test_deterministic_and_batch_invariant(build, net, fixture):
    audio, video = fixture["audio"].to(DEV), fixture["video"].to(DEV)
    s1, s2 = net(audio, video), net(audio, video)
    assert torch.equal(s1, s2)
    singles = torch.cat([net(audio[i:i + 1], video[i:i + 1]) for i in range(2)])
    assert torch.equal(s1, singles)
    assert torch.equal(net.embed_video(video), torch.cat([net.embed_video(video[i:i + 1]) for i in range(2)]))


def test_both_builds_agree_bit_for_bit(net, fixture):
    """the point of the f32 path: the metric does not depend on the storage type the library was built for"""
    from asva_amd import avsync as A

    _both_built()
    audio, video = fixture["audio"].to(DEV), fixture["video"].to(DEV)
    frames = R.u8_to_unit(load_golden("avsync_preprocess.pt")["frames_u8"]).permute(1, 0, 2, 3)[None].to(DEV)

    def run():
        return net.embed_audio(audio).clone(), net.embed_video(video).clone(), net(audio, video).clone(), A.preprocess_videos(frames).clone()

    for x, y in zip(_in_build("bf16", run), _in_build("fp16", run)):
        assert torch.equal(x, y)


def test_sync_metrics_end_to_end(build, net):
    from asva_amd import avsync as A
    from asva_amd.audio_features import waveform_to_melspectrogram

    t = torch.arange(32000, dtype=torch.float32) / 16000.0
    wave = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) * (1.0 + torch.sin(2 * torch.pi * 3.0 * t)))[None]
    wave2 = (0.2 * torch.sin(2 * torch.pi * 1200.0 * t * (1.0 + 0.2 * t)))[None]
    clip = R.u8_to_unit(R.grating_video_u8(12, 256, 256, 0.7, 0.13, 23.0))
    clip2 = R.u8_to_unit(R.grating_video_u8(12, 256, 256, 2.2, -0.3, 41.0, mean=0.4, contrast=0.3))
    score = A.compute_sync_metrics_on_av(wave, 16000, clip, metric="avsync_score", net=net)
    rel_v = A.compute_sync_metrics_on_av(wave, 16000, clip, ref_video=clip2, metric="relsync", net=net)
    rel_a = A.compute_sync_metrics_on_av(wave, 16000, clip, ref_audio_waveform=wave2, metric="relsync", net=net)
    assert all(bool(torch.isfinite(v)) for v in (score, rel_v, rel_a)) and 0.0 < float(rel_v) < 1.0 and 0.0 < float(rel_a) < 1.0
    # equals the composed calls
    mel, mel2 = (waveform_to_melspectrogram(w, device=DEV)[None] for w in (wave, wave2))
    vid, vid2 = A.preprocess_videos(clip[None].to(DEV)), A.preprocess_videos(clip2[None].to(DEV))
    s, s_v, s_a = net(mel, vid), net(mel, vid2), net(mel2, vid)
    assert torch.equal(score, s[0])
    assert torch.equal(rel_v, A.relsync_from_scores(s_v, s).cpu()[0]) and torch.equal(rel_a, A.relsync_from_scores(s_a, s).cpu()[0])
    with pytest.raises(ValueError, match="16000"):
        A.compute_sync_metrics_on_av(wave, 44100, clip, metric="avsync_score", net=net)


def test_avsync_score_tool_runs():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "avsync_score.py"), "--clips", "1", "--steps", "2"],
                       capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "RelSync" in r.stdout and "mean nothing" in r.stdout
