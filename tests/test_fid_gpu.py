"""FID on the MI355X (asva_amd/fid.py, asva_amd/evaluation.py; kernels in csrc/avsync.hip), in both builds of the library.

Bounds (none comes from what the kernels give):
  * avsd_convnd_ld_f32 is avsd_convnd_f32 with other addresses: torch.equal against the dense kernel on contiguous copies; against
    float64 the bound of tests/test_avsync_gpu.py::test_convnd_f32_against_float64, rel-L2 < 1e-6;
  * avsd_pool3_hw_f32: the maximum is exact (torch.equal); the average is at most 9 additions and one division in f32, rel-L2 < 1e-6;
  * preprocessing: the bound of tests/test_avsync_gpu.py::test_resize_normalize_against_fixture (tests/golden/avsync_measured.json);
  * whole extractor: 4 x the rel-L2 of torch's own float32 CPU forward against the float64 restatement on the fixture (the reference's
    arithmetic; tests/golden/fid/measured.json "cpu", written by tools/gen_fid_golden.py), capped at 1e-4;
  * determinism, batch / chunk invariance, build invariance, the driver against directly computed values: exact.
Measured on MI355X: tests/golden/fid/measured.json, "gpu".
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import avsync_ref as AR
from tests import inception_ref as R
from tests.helpers import GOLDEN, ROOT, load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0


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


def _measured():
    with open(os.path.join(GOLDEN, "fid", "measured.json")) as f:
        return json.load(f)


def _net_bound():
    return min(4.0 * _measured()["cpu"]["f32_vs_f64_rel_l2"], 1e-4)


@pytest.fixture(scope="module")
def fixture():
    g = load_golden(os.path.join("fid", "fid_tiny.pt"))
    sd = R.draw_state_dict(load_shapes(os.path.join("fid", "state_dict_shapes.json")), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    g["inputs"] = [R.preprocess(R.u8_to_unit(img)[None]) for img in g["images_u8"]]       # float32, as the generator fed the restatement
    return g


@pytest.fixture(scope="module")
def net(fixture):
    from asva_amd import fid

    m = fid.InceptionV3((3, 4))
    m.load_state_dict(fixture["sd"])
    return m.to(DEV)


@pytest.fixture(scope="module")
def second_draw(fixture):
    """inputs the fixture does not hold, and their float64 restatement (computed once, shared by both builds)"""
    g = torch.Generator().manual_seed(11)
    x = torch.stack([R.u8_to_unit(R.image_u8(99, 83, 0.7 + i, 9.0 + 8.0 * i, seed=20 + i)) for i in range(2)]) * 2 - 1
    x = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(-1, 1)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in fixture["sd"].items()}
    with torch.no_grad():
        feat, logits = R.forward(sd64, x.double())
    return x, feat, logits


# ---- avsd_convnd_ld_f32 ------------------------------------------------------------------------------------------------------------------
# (name, (kh, kw), stride, (ph, pw), cin, cout, (h, w), channel offset and width of the input buffer, the same for the output buffer)
LD_CASES = [
    ("1x1_288to64_in_slice_at_64_of_352", (1, 1), 1, (0, 0), 288, 64, (12, 12), (64, 352), (0, 64)),
    ("1x7_128to128", (1, 7), 1, (0, 3), 128, 128, (12, 12), (128, 256), (192, 768)),
    ("7x1_128to128", (7, 1), 1, (3, 0), 128, 128, (12, 12), (0, 256), (0, 128)),
    ("5x5_p2_48to64_scalar", (5, 5), 1, (2, 2), 48, 64, (13, 9), (0, 112), (64, 224)),
    ("3x3_s2_288to384_out_at_0_of_768", (3, 3), 2, (0, 0), 288, 384, (13, 11), (0, 288), (0, 768)),
    ("1x3_384to384_first_half_of_768", (1, 3), 1, (0, 1), 384, 384, (5, 5), (0, 832), (320, 2048)),
    ("3x1_384to384_second_half_of_768", (3, 1), 1, (1, 0), 384, 384, (5, 5), (0, 832), (704, 2048)),
    ("3x3_s2_3to32_on_75x91", (3, 3), 2, (0, 0), 3, 32, (75, 91), (1, 4), (0, 32)),
    ("3x3_80to192_of_96_wide", (3, 3), 1, (0, 0), 80, 192, (9, 9), (0, 96), (0, 192)),
    ("3x3_p1_448to384_m50", (3, 3), 1, (1, 1), 448, 384, (5, 5), (384, 832), (0, 384)),
]


def _ld_case(case, seed=0):
    name, (kh, kw), s, (ph, pw), cin, cout, (h, w), (xo, ldx), (yo, ldy) = case
    n = 2
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    bias = torch.randn(cout, generator=g)
    k = cin * kh * kw
    wp = torch.zeros(cout, (k + 3) // 4 * 4)
    wp[:, :k] = wt.permute(0, 2, 3, 1).reshape(cout, k)
    xw = torch.full((n, 1, h, w, ldx), float("nan"))                      # every gap of the wide input is NaN
    xw[..., xo:xo + cin] = x.permute(0, 2, 3, 1).unsqueeze(1)
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    yw = torch.full((n, 1, ho, wo, ldy), SENTINEL)
    return x, wt, bias, wp, xw, yw


@pytest.mark.parametrize("case", LD_CASES, ids=[c[0] for c in LD_CASES])
def test_convnd_ld_is_the_dense_conv_bit_for_bit_and_exact_f32(build, case):
    from asva_amd import ops

    name, (kh, kw), s, (ph, pw), cin, cout, (h, w), (xo, ldx), (yo, ldy) = case
    x, wt, bias, wp, xw, yw = _ld_case(case)
    xw, yw, wd, bd = xw.to(DEV), yw.to(DEV), wp.to(DEV), bias.to(DEV)
    taps, stride, pad = (1, kh, kw), (1, s, s), (0, ph, pw)
    xs, ys = xw[..., xo:xo + cin], yw[..., yo:yo + cout]
    got = ops.convnd_ld_f32(xs, wd, taps, stride, pad, out=ys, bias=bd, relu=True)
    assert got.data_ptr() == ys.data_ptr()
    dense = ops.convnd_f32(xs.contiguous(), wd, taps, stride, pad, bias=bd, relu=True)
    assert torch.equal(ys, dense), name
    # nothing outside the slice was written, and no NaN of the gaps was read
    outside = torch.ones(ldy, dtype=torch.bool, device=DEV)
    outside[yo:yo + cout] = False
    assert bool((yw[..., outside] == SENTINEL).all()) and bool(torch.isfinite(ys).all())
    # without an `out`: a fresh dense tensor with the same bits
    assert torch.equal(ops.convnd_ld_f32(xs, wd, taps, stride, pad, bias=bd, relu=True), dense)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), s, (ph, pw)).relu()
    err = R.rel_l2(ys[:, 0].permute(0, 3, 1, 2), ref)
    print(f"convnd_ld_f32 {name} [{build}]: rel-L2 against float64 {err:.3e}")
    assert err < 1e-6, (name, err)


def test_convnd_ld_residual_is_read_with_ldy(build):
    """include/avsd.h: res has the layout of out.  A residual held in a slice of one wide buffer, the output written to another
    slice of a buffer of the same width: the bits of the dense kernel with the same residual and per-channel scale"""
    from asva_amd import ops

    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1, 7, 5, 64, generator=g).to(DEV)
    w = (torch.randn(96, 9 * 64, generator=g) / 24.0).to(DEV)
    bias, rscale = torch.randn(96, generator=g).to(DEV), (0.5 + torch.rand(96, generator=g)).to(DEV)
    res = torch.randn(2, 1, 7, 5, 96, generator=g).to(DEV)
    args = ((1, 3, 3), (1, 1, 1), (0, 1, 1))
    dense = ops.convnd_f32(x, w, *args, bias=bias, res=res, rscale=rscale, relu=True)
    rw = torch.full((2, 1, 7, 5, 224), float("nan"), device=DEV)
    rw[..., 128:224] = res
    yw = torch.full((2, 1, 7, 5, 224), SENTINEL, device=DEV)
    ops.convnd_ld_f32(x, w, *args, out=yw[..., 32:128], bias=bias, res=rw[..., 128:224], rscale=rscale, relu=True)
    assert torch.equal(yw[..., 32:128], dense)
    assert bool((yw[..., :32] == SENTINEL).all()) and bool((yw[..., 128:] == SENTINEL).all())
    with pytest.raises(ValueError, match="pixel stride"):
        ops.convnd_ld_f32(x, w, *args, out=yw[..., 32:128], res=res)            # a dense residual for a strided output


def test_convnd_ld_refuses_bad_strides_and_falls_back_on_misaligned_slices(build):
    from asva_amd import _lib, ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 6, 6, 32, generator=g).to(DEV)
    w = (torch.randn(32, 9 * 32, generator=g) / 17.0).to(DEV)
    args = ((1, 3, 3), (1, 1, 1), (0, 1, 1))
    dense = ops.convnd_f32(x, w, *args)
    with pytest.raises(_lib.AvsdError, match="ldx"):
        ops.convnd_ld_f32(x, w, *args, ldx=31)
    with pytest.raises(_lib.AvsdError, match="ldy"):
        ops.convnd_ld_f32(x, w, *args, ldy=31)
    with pytest.raises(ValueError):
        ops.convnd_ld_f32(x, w, *args, ldx=64)                                  # wider than the memory behind the view
    with pytest.raises(ValueError):
        ops.convnd_ld_f32(x.permute(0, 1, 3, 2, 4), w, *args)                    # not a channel slice of a channels-last buffer
    with pytest.raises(ValueError):
        ops.convnd_ld_f32(x, w, *args, out=torch.empty(2, 1, 6, 5, 32, device=DEV))
    # documented in include/avsd.h: a slice the float4 loader cannot read (start not 16-byte aligned, or ldx not a multiple of 4)
    # falls back to the scalar loader, with the same bits
    for off, ld in ((2, 36), (0, 34), (1, 34)):
        wide = torch.full((2, 1, 6, 6, ld), float("nan"), device=DEV)
        wide[..., off:off + 32] = x
        assert torch.equal(ops.convnd_ld_f32(wide[..., off:off + 32], w, *args), dense), (off, ld)


# ---- avsd_pool3_hw_f32 -------------------------------------------------------------------------------------------------------------------
POOL_MODES = [("max", 2, 0), ("avg", 1, 1), ("max", 1, 1)]
POOL_SHAPES = [(12, 12), (13, 9), (5, 5), (3, 3), (1, 1)]


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("c", [8, 288])
@pytest.mark.parametrize("mode,stride,pad", POOL_MODES, ids=["max_s2_p0", "avg_s1_p1", "max_s1_p1"])
def test_pool3(build, mode, stride, pad, c, sliced):
    from asva_amd import ops

    for h, w in POOL_SHAPES:
        x = torch.randn(2, c, h, w, generator=torch.Generator().manual_seed(h * 100 + w + c))
        if stride == 2 and min(h, w) < 3:                                       # 3 x 3 is the smallest legal input of the stride-2 pool
            with pytest.raises(ValueError):
                ops.pool3_hw_f32(x.permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(DEV), mode, stride, pad)
            continue
        xo, ldx, yo, ldy = (4, c + 12, 8, c + 16) if sliced else (0, c, 0, c)
        xw = torch.full((2, 1, h, w, ldx), float("nan"))
        xw[..., xo:xo + c] = x.permute(0, 2, 3, 1).unsqueeze(1)
        ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
        yw = torch.full((2, 1, ho, wo, ldy), SENTINEL).to(DEV)
        ys = yw[..., yo:yo + c]
        ops.pool3_hw_f32(xw.to(DEV)[..., xo:xo + c], mode, stride, pad, out=ys)
        got = ys[:, 0].permute(0, 3, 1, 2).cpu()
        outside = torch.ones(ldy, dtype=torch.bool)
        outside[yo:yo + c] = False
        assert bool((yw.cpu()[..., outside] == SENTINEL).all())
        if mode == "max":
            assert torch.equal(got, F.max_pool2d(x, 3, stride, pad)), (h, w)
        else:
            err = R.rel_l2(got, F.avg_pool2d(x.double(), 3, stride, pad, count_include_pad=False))
            assert err < 1e-6, (h, w, err)
        if not sliced:
            assert torch.equal(ops.pool3_hw_f32(xw.to(DEV), mode, stride, pad), ys)


def test_pool3_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    x = torch.zeros(1, 1, 5, 5, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.pool3_hw_f32(x, "min", 1, 1)
    with pytest.raises(ValueError):
        ops.pool3_hw_f32(x, "max", 1, 1, out=torch.zeros(1, 1, 4, 5, 8, device=DEV))
    with pytest.raises(_lib.AvsdError, match="stride"):
        ops.pool3_hw_f32(x, "max", 2, 1)
    with pytest.raises(_lib.AvsdError, match="multiple of 4"):
        ops.pool3_hw_f32(torch.zeros(1, 1, 5, 5, 6, device=DEV), "max", 1, 1)


# ---- preprocessing -------------------------------------------------------------------------------------------------------------------------
def _resize_bound():
    with open(os.path.join(GOLDEN, "avsync_measured.json")) as f:
        m = json.load(f)
    return min(4.0 * m["cpu"]["resize_tables_max_abs"], 1e-5)


def test_preprocess_images_against_torch(build, fixture):
    from asva_amd import fid

    for img, want in zip(fixture["images_u8"], fixture["inputs"]):
        out = fid.preprocess_images(R.u8_to_unit(img)[None].to(DEV))
        assert out.shape == (1, 3, 229, 229)
        err = (out.cpu() - want).abs().max().item()
        print(f"preprocess_images {tuple(img.shape)} [{build}]: max abs {err:.3e} (bound {_resize_bound():.3e})")
        assert err <= _resize_bound()


# ---- the whole extractor -------------------------------------------------------------------------------------------------------------------
def test_extractor_against_fixture(build, net, fixture):
    bound = _net_bound()
    for i, x in enumerate(fixture["inputs"]):
        st = {}
        feat, logits = net(x.to(DEV), stages=st)
        assert feat.shape == (1, 2048) and logits.shape == (1, 1008)
        ef, el = R.rel_l2(feat[0], fixture["features"][i]), R.rel_l2(logits[0], fixture["logits"][i])
        print(f"extractor vs fixture, image {i} {tuple(fixture['images_u8'][i].shape)} [{build}]: features rel-L2 {ef:.3e}, "
              f"logits {el:.3e} (bound {bound:.3e})")
        worst = 0.0
        for name in R.STAGES:                                                   # localises a wrong layer
            e = R.rel_l2(st[name][0, 0].double().mean(dim=(0, 1)), fixture["stage_means"][name][i])
            worst = max(worst, e)
            assert e <= bound, (name, i, e)
        print(f"  worst stage position mean: rel-L2 {worst:.3e}")
        assert ef <= bound and el <= bound


def test_extractor_against_restatement(build, net, second_draw):
    from asva_amd import fid

    x, feat_ref, logits_ref = second_draw
    feat, logits = net(x.to(DEV))
    ef, el = R.rel_l2(feat, feat_ref), R.rel_l2(logits, logits_ref)
    print(f"extractor vs restatement {tuple(x.shape)} [{build}]: features rel-L2 {ef:.3e}, logits {el:.3e} (bound {_net_bound():.3e})")
    assert ef <= _net_bound() and el <= _net_bound()
    # the reference's forward: requested blocks ascending, blocks 0 - 2 as NCHW maps
    maps = fid.InceptionV3((2, 0, 1))
    maps.load_state_dict(net.state_dict())
    b0, b1, b2 = maps.to(DEV)(x.to(DEV))
    assert b0.shape == (2, 64, 23, 19) and b1.shape == (2, 192, 10, 8) and b2.shape == (2, 768, 4, 3)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 74, 80, device=DEV))


def _small_images(n=3):
    return torch.stack([R.u8_to_unit(R.image_u8(96, 80, 0.4 + 0.9 * i, 11.0 + 6.0 * i, seed=30 + i)) for i in range(n)])


def test_deterministic_batch_and_chunk_invariant(build, net):
    from asva_amd import fid

    images = _small_images().to(DEV)
    a, b = fid.compute_fid_image_features(images, net), fid.compute_fid_image_features(images, net)
    assert a.shape == (3, 2048) and torch.equal(a, b)
    singles = torch.cat([fid.compute_fid_image_features(images[i:i + 1], net) for i in range(3)])
    assert torch.equal(a, singles)
    assert torch.equal(a, fid.compute_fid_image_features(images, net, chunk=2))      # a batch larger than the chunk
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])


def test_both_builds_agree_bit_for_bit(net):
    from asva_amd import _lib, fid

    if not all(os.path.isfile(p) for p in _lib.LIB_PATHS.values()):
        pytest.skip("needs both the bf16 and the fp16 library")
    images = _small_images(2).to(DEV)

    def run():
        x = fid.preprocess_images(images)
        feat, logits = net(x)
        return x.clone(), feat.clone(), logits.clone()

    for x, y in zip(_in_build("bf16", run), _in_build("fp16", run)):
        assert torch.equal(x, y)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
FRAMES, FPS, SIZE, NCLIPS = 3, 6, 96, 2


def _write_dataset(root):
    """2 groundtruth videos (2 s at 6 fps, 96 x 96, 16 kHz audio) and, per groundtruth clip, one generated clip of 3 frames, in the
    pre-decoded clip container of asva_amd.data_utils"""
    rng = np.random.default_rng(0)
    names = ["beta.npz", "alpha.npz"]                                            # unsorted: the driver sorts
    (root / "gt").mkdir()
    (root / "gen").mkdir()
    for n in names:
        base = rng.integers(0, 255, (12, 12, 12, 3), dtype=np.uint8)
        frames = np.repeat(np.repeat(base, 8, 1), 8, 2)                          # (12, 96, 96, 3), blocks that change every frame
        audio = (rng.standard_normal((1, 2 * 16000)) * 0.1).astype(np.float32)
        np.savez(root / "gt" / n, frames=frames, fps=6.0, audio=audio, audio_sr=16000)
        for k in range(NCLIPS):
            gen = np.repeat(np.repeat(rng.integers(0, 255, (FRAMES, 6, 6, 3), dtype=np.uint8), 16, 1), 16, 2)
            a = (rng.standard_normal((1, 8000)) * 0.1).astype(np.float32)
            np.savez(root / "gen" / (n[:-4] + f"_clip-{k:02d}.npz"), frames=gen, fps=6.0, audio=a, audio_sr=16000)
    return names


def test_driver_fid_and_relsync_equal_direct_computation(build, net, fixture, tmp_path):
    from asva_amd import avsync as A
    from asva_amd import fid
    from asva_amd.data_utils import load_av_clips_uniformly
    from avgen.evaluations.eval import evaluate_generation_results

    g = load_golden("avsync_tiny.pt")
    sd = AR.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    AR.check_draw(sd, g["probe"])
    sync = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    sync.load_state_dict(sd)
    inception = fid.InceptionV3((3,))
    inception.load_state_dict(fixture["sd"])
    names = _write_dataset(tmp_path)
    out = tmp_path / "results" / "metrics.json"
    common = dict(groundtruth_video_root=str(tmp_path / "gt"), groundtruth_video_names=list(names), groundtruth_categories=["dog", "cat"],
                  num_clips_per_video=NCLIPS, generated_video_root=str(tmp_path / "gen"), result_save_path=str(out), image_size=SIZE,
                  video_fps=FPS, video_num_frame=FRAMES)
    with pytest.raises(NotImplementedError, match="eval_fvd=False"):
        evaluate_generation_results(**common, models={"fid": inception, "avsync": sync})
    res = evaluate_generation_results(**common, eval_fid=True, eval_fvd=False, eval_clipsim=False, eval_relsync=True, eval_alignsync=False,
                                      record_instance_metrics=True, models={"fid": inception, "avsync": sync})
    with open(out) as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(res))
    assert sorted(saved) == sorted(["groundtruth_video_root", "generated_video_root", "num_clips_per_video", "FID", "RelSync_mean",
                                    "RelSync_std", "instance_metrics"])
    # directly: groundtruth clips in sorted order, the generated clips of each in sorted order, the first frame dropped
    gt_v, gt_a, gen_v, gen_a, gen_names = [], [], [], [], []
    for n in sorted(names):
        v, a = load_av_clips_uniformly(str(tmp_path / "gt" / n), FPS, FRAMES, SIZE, NCLIPS)
        gt_v.append(v), gt_a.append(a)
        for k in range(NCLIPS):
            gen_names.append(n[:-4] + f"_clip-{k:02d}.npz")
            v, a = load_av_clips_uniformly(str(tmp_path / "gen" / gen_names[-1]), FPS, FRAMES, SIZE, 1)
            gen_v.append(v), gen_a.append(a)
    gt_v, gen_v = torch.cat(gt_v).to(DEV), torch.cat(gen_v).to(DEV)             # (4, 3, 3, 96, 96)
    gt_a, gen_a = torch.cat(gt_a).to(DEV), torch.cat(gen_a).to(DEV)
    assert gt_v.shape == (4, FRAMES, 3, SIZE, SIZE) and gen_v.shape == gt_v.shape

    def feats(v):
        return fid.compute_fid_image_features(v[:, 1:].flatten(end_dim=1), inception).cpu()

    want_fid = fid.frechet_distance(feats(gt_v), feats(gen_v)).item()
    s_gt = A.compute_avsync_scores(gt_a, gt_v.permute(0, 2, 1, 3, 4), sync).cpu()
    s_gen = A.compute_avsync_scores(gen_a, gen_v.permute(0, 2, 1, 3, 4), sync).cpu()
    rel = torch.exp(s_gen) / (torch.exp(s_gt) + torch.exp(s_gen))
    print(f"driver [{build}]: FID {saved['FID']:.6f} (direct {want_fid:.6f}), RelSync_mean {saved['RelSync_mean']:.6f} (direct {rel.mean().item():.6f})")
    assert saved["FID"] == want_fid and saved["FID"] > 0.0
    assert saved["RelSync_mean"] == rel.mean().item() and saved["RelSync_std"] == rel.std().item()
    assert list(saved["instance_metrics"]) == gen_names
    assert [saved["instance_metrics"][n]["RelSync"] for n in gen_names] == [r.item() for r in rel]
    # a missing generated clip is the reference's assertion
    os.remove(tmp_path / "gen" / gen_names[0])
    with pytest.raises(AssertionError, match="does not equal to num_clips_per_video"):
        evaluate_generation_results(**common, eval_fvd=False, eval_clipsim=False, eval_alignsync=False, models={"fid": inception, "avsync": sync})


def test_fid_score_tool_runs():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "fid_score.py")], capture_output=True,
                       text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "FID:" in r.stdout and "means nothing" in r.stdout
