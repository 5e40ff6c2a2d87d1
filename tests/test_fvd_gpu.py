"""FVD on the MI355X (asva_amd/fvd.py, asva_amd/evaluation.py; kernels in csrc/avsync.hip), in both builds of the library.

Bounds (none comes from what the kernels give):
  * avsd_conv3d_same_f32 against F.conv3d(F.pad(x, same padding)) in float64: the bound of
    tests/test_avsync_gpu.py::test_convnd_f32_against_float64, rel-L2 < 1e-6; against avsd_convnd_ld_f32 / avsd_convnd_f32 where the
    padding is symmetric, between its loaders, and between dense tensors and channel slices: torch.equal;
  * avsd_maxpool3d_same_f32 is exact: torch.equal against F.max_pool3d(F.pad(x, same padding));
  * preprocessing: the bound of tests/test_avsync_gpu.py::test_resize_normalize_against_fixture (tests/golden/avsync_measured.json);
  * whole extractor: 4 x the rel-L2 of the reference module's own float32 CPU forward against its float64 forward on the fixture
    (tests/golden/fvd/measured.json "cpu", written by tools/gen_fvd_golden.py), capped at 1e-4;
  * determinism, batch / chunk invariance, build invariance, the driver against directly computed values: exact.
Measured on MI355X: tests/golden/fvd/measured.json, "gpu".
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import avsync_ref as AR
from tests import i3d_ref as R
from tests.helpers import GOLDEN, ROOT, load_golden, load_shapes
from tests.test_fid_gpu import DEV, SENTINEL, _in_build, _resize_bound, build  # noqa: F401  (`build`: the fixture of both libraries)

pytestmark = pytest.mark.gpu

GUARD = 1024          # floats of NaN before and behind an input: a read outside the tensor shows


def _measured():
    with open(os.path.join(GOLDEN, "fvd", "measured.json")) as f:
        return json.load(f)


def _net_bound():
    return min(4.0 * _measured()["cpu"]["f32_vs_f64_rel_l2"], 1e-4)


@pytest.fixture(scope="module")
def fixture():
    g = load_golden(os.path.join("fvd", "fvd_tiny.pt"))
    sd = R.draw_state_dict(load_shapes(os.path.join("fvd", "state_dict_shapes.json")), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    g["inputs"] = [R.preprocess(R.clip_to_bcthw(c)) for c in g["clips_u8"]]       # float32, as the generator fed the reference module
    return g


@pytest.fixture(scope="module")
def net(fixture):
    from asva_amd import fvd

    m = fvd.InceptionI3d()
    m.load_state_dict(fixture["sd"])
    return m.to(DEV)


def _guarded(t):
    """t on the device, in the middle of a larger NaN-filled allocation"""
    big = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV)
    big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return big[GUARD:GUARD + t.numel()].view(t.shape)


# ---- avsd_conv3d_same_f32 ----------------------------------------------------------------------------------------------------------------
# (name, window, stride, cin, cout, (t, h, w)); two samples each.  The last two are the smallest shapes that take the 128 x 64 and the
# 128 x 128 tile (the tile rule of avsd_convnd_f32: at least 256 tiles of 128 rows)
CONV_CASES = [
    ("stem_7x7x7_s2_3to64_even", (7, 7, 7), (2, 2, 2), 3, 64, (6, 18, 14)),
    ("stem_7x7x7_s2_3to64_odd", (7, 7, 7), (2, 2, 2), 3, 64, (5, 17, 13)),
    ("7x7x7_s1_3to64", (7, 7, 7), (1, 1, 1), 3, 64, (5, 9, 8)),
    ("3x3x3_s1_32to208_m210", (3, 3, 3), (1, 1, 1), 32, 208, (3, 7, 5)),
    ("3x3x3_s2_32to208_m48", (3, 3, 3), (2, 2, 2), 32, 208, (3, 7, 5)),
    ("3x3x3_s1_64to48_m432", (3, 3, 3), (1, 1, 1), 64, 48, (4, 6, 9)),
    ("3x3x3_s2_64to48_m60", (3, 3, 3), (2, 2, 2), 64, 48, (4, 6, 9)),
    ("1x1x1_96to64", (1, 1, 1), (1, 1, 1), 96, 64, (3, 7, 5)),
    ("stem_7x7x7_s2_3to64_tile_128x64", (7, 7, 7), (2, 2, 2), 3, 64, (8, 128, 130)),
    ("3x3x3_s1_32to208_tile_128x128", (3, 3, 3), (1, 1, 1), 32, 208, (4, 48, 43)),
]
CONV_BY_NAME = {c[0]: c for c in CONV_CASES}


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    """inputs and the float64 reference of one case, computed once and shared by both builds and all tests"""
    _, k, s, cin, cout, thw = CONV_BY_NAME[name]
    g = torch.Generator().manual_seed(len(name) + cin)
    x = torch.randn(2, cin, *thw, generator=g)
    kk = cin * k[0] * k[1] * k[2]
    wt = torch.randn(cout, cin, *k, generator=g) * (2.0 / kk) ** 0.5
    bias = torch.randn(cout, generator=g)
    wp = torch.zeros(cout, (kk + 3) // 4 * 4)
    wp[:, :kk] = wt.permute(0, 2, 3, 4, 1).reshape(cout, kk)
    ref = F.conv3d(R.pad_same(x.double(), k, s), wt.double(), bias.double(), s).relu()
    assert tuple(ref.shape[2:]) == tuple(-(-d // st) for d, st in zip(thw, s))
    return x.permute(0, 2, 3, 4, 1).contiguous(), wp, bias, ref


@pytest.mark.parametrize("name", [c[0] for c in CONV_CASES])
def test_conv3d_same_against_float64_dense_and_as_slices(build, name):
    from asva_amd import ops

    _, k, s, cin, cout, thw = CONV_BY_NAME[name]
    x, wp, bias, ref = _conv_case(name)
    wd, bd = wp.to(DEV), bias.to(DEV)
    dense = ops.conv3d_same_f32(_guarded(x), wd, k, s, bias=bd, relu=True)
    err = R.rel_l2(dense.permute(0, 4, 1, 2, 3), ref)
    print(f"conv3d_same_f32 {name} [{build}]: rel-L2 against float64 {err:.3e}")
    assert tuple(dense.shape) == (2, *ref.shape[2:], cout) and err < 1e-6, (name, err)
    # as channel slices: the gaps of the wide input hold NaN, the output buffer a sentinel
    xo, ldx, yo, ldy = (1 if cin % 4 else 4), cin + (5 if cin % 4 else 12), 8, cout + 16
    xw = torch.full((*x.shape[:4], ldx), float("nan"))
    xw[..., xo:xo + cin] = x
    xs = _guarded(xw)[..., xo:xo + cin]
    yw = torch.full((*dense.shape[:4], ldy), SENTINEL, device=DEV)
    ys = yw[..., yo:yo + cout]
    got = ops.conv3d_same_f32(xs, wd, k, s, out=ys, bias=bd, relu=True)
    assert got.data_ptr() == ys.data_ptr() and torch.equal(ys, dense), name
    outside = torch.ones(ldy, dtype=torch.bool, device=DEV)
    outside[yo:yo + cout] = False
    assert bool((yw[..., outside] == SENTINEL).all()) and bool(torch.isfinite(ys).all())
    if s == (1, 1, 1):                                                          # symmetric padding: the bits of avsd_convnd_ld_f32
        pad = tuple((kk - 1) // 2 for kk in k)
        assert torch.equal(ops.convnd_ld_f32(xs, wd, k, s, pad, bias=bd, relu=True), dense), name


@pytest.mark.parametrize("name", ["stem_7x7x7_s2_3to64_even", "stem_7x7x7_s2_3to64_odd", "7x7x7_s1_3to64", "3x3x3_s2_32to208_m48",
                                  "3x3x3_s1_64to48_m432", "stem_7x7x7_s2_3to64_tile_128x64"])
def test_conv3d_same_loaders_give_the_same_bits(build, name):
    from asva_amd import _lib, ops

    _, k, s, cin, cout, thw = CONV_BY_NAME[name]
    x, wp, bias, _ = _conv_case(name)
    xd, wd, bd = _guarded(x), wp.to(DEV), bias.to(DEV)
    auto = ops.conv3d_same_f32(xd, wd, k, s, bias=bd, relu=True)
    legal = (1, 2, 3) if cin % 32 == 0 else (1, 3)
    for loader in legal:
        assert torch.equal(ops.conv3d_same_f32(xd, wd, k, s, bias=bd, relu=True, loader=loader), auto), (name, loader)
    if 2 not in legal:
        with pytest.raises(_lib.AvsdError, match="loader 2"):
            ops.conv3d_same_f32(xd, wd, k, s, loader=2)
    if name == "7x7x7_s1_3to64":
        assert torch.equal(ops.convnd_f32(xd, wd, k, s, (3, 3, 3), bias=bd, relu=True), auto)


def test_conv3d_same_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    x = torch.zeros(1, 4, 6, 6, 32, device=DEV)
    w = torch.zeros(16, 27 * 32, device=DEV)
    with pytest.raises(ValueError, match="does not match"):
        ops.conv3d_same_f32(x, w, (3, 3, 3), (2, 2, 2), out=torch.zeros(1, 2, 3, 2, 16, device=DEV))      # ceil(6 / 2) = 3
    with pytest.raises(_lib.AvsdError, match="loader must be"):
        ops.conv3d_same_f32(x, w, (3, 3, 3), (2, 2, 2), loader=5)
    wide = torch.zeros(1, 4, 6, 6, 64, device=DEV)
    with pytest.raises(_lib.AvsdError, match="loader 3"):
        ops.conv3d_same_f32(wide[..., :32], w, (3, 3, 3), (2, 2, 2), loader=3)                               # pixels are not side by side
    with pytest.raises(_lib.AvsdError, match="ldx"):
        ops.conv3d_same_f32(x, w, (3, 3, 3), (2, 2, 2), ldx=31)
    with pytest.raises(_lib.AvsdError, match="ldw"):
        ops.conv3d_same_f32(x, w[:, :-4].contiguous(), (3, 3, 3), (2, 2, 2))


# ---- avsd_maxpool3d_same_f32 -------------------------------------------------------------------------------------------------------------
POOL_KINDS = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1))]
POOL_SHAPES = [(2, 9, 8), (2, 8, 7), (6, 8, 8), (5, 7, 9), (3, 14, 14), (3, 7, 7), (1, 1, 1)]


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("c", [8, 528])
@pytest.mark.parametrize("k,s", POOL_KINDS, ids=["1x3x3_s122", "3x3x3_s2", "2x2x2_s2", "3x3x3_s1"])
def test_maxpool3d_same(build, k, s, c, sliced):
    from asva_amd import ops

    for thw in POOL_SHAPES:
        x = torch.randn(2, c, *thw, generator=torch.Generator().manual_seed(sum(thw) * 100 + c))       # negative values: a padded 0 shows
        want = F.max_pool3d(R.pad_same(x, k, s), k, s)
        xo, ldx, yo, ldy = (4, c + 12, 8, c + 16) if sliced else (0, c, 0, c)
        xw = torch.full((2, *thw, ldx), float("nan"))
        xw[..., xo:xo + c] = x.permute(0, 2, 3, 4, 1)
        yw = torch.full((2, *want.shape[2:], ldy), SENTINEL, device=DEV)
        ys = yw[..., yo:yo + c]
        ops.maxpool3d_same_f32(_guarded(xw)[..., xo:xo + c], k, s, out=ys)
        outside = torch.ones(ldy, dtype=torch.bool, device=DEV)
        outside[yo:yo + c] = False
        assert bool((yw[..., outside] == SENTINEL).all())
        assert torch.equal(ys.permute(0, 4, 1, 2, 3).cpu(), want), (k, s, thw)
        if not sliced:
            assert torch.equal(ops.maxpool3d_same_f32(xw.to(DEV), k, s), ys)


def test_maxpool3d_same_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    x = torch.zeros(1, 3, 5, 5, 8, device=DEV)
    with pytest.raises(ValueError, match="does not match"):
        ops.maxpool3d_same_f32(x, (3, 3, 3), (2, 2, 2), out=torch.zeros(1, 1, 3, 3, 8, device=DEV))
    with pytest.raises(_lib.AvsdError, match="windows must be 1 .. 3"):
        ops.maxpool3d_same_f32(x, (1, 4, 4), (1, 1, 1))
    with pytest.raises(_lib.AvsdError, match="strides must be 1 .. 2"):
        ops.maxpool3d_same_f32(x, (3, 3, 3), (3, 3, 3))
    with pytest.raises(_lib.AvsdError, match="multiple of 4"):
        ops.maxpool3d_same_f32(torch.zeros(1, 3, 5, 5, 6, device=DEV), (3, 3, 3), (1, 1, 1))


# ---- preprocessing -------------------------------------------------------------------------------------------------------------------------
def test_preprocess_videos_against_torch(build, fixture):
    from asva_amd import fvd

    for clip, want in zip(fixture["clips_u8"], fixture["inputs"]):
        out = fvd.preprocess_videos(R.clip_to_bcthw(clip).to(DEV))
        assert out.shape == (1, 3, clip.shape[0], 224, 224)
        assert out.permute(0, 2, 3, 4, 1).is_contiguous()                       # channels-last memory: the network reads it without a copy
        err = (out.cpu() - want).abs().max().item()
        print(f"preprocess_videos {tuple(clip.shape)} [{build}]: max abs {err:.3e} (bound {_resize_bound():.3e})")
        assert err <= _resize_bound()
    cropped = fvd.preprocess_videos(R.clip_to_bcthw(fixture["clips_u8"][1]).to(DEV), sequence_length=9)
    assert cropped.shape == (1, 3, 9, 224, 224) and torch.equal(cropped, out[:, :, :9])


# ---- the whole extractor -------------------------------------------------------------------------------------------------------------------
def test_extractor_against_fixture(build, net, fixture):
    bound = _net_bound()
    for i, x in enumerate(fixture["inputs"]):
        st = {}
        feat = net(x.to(DEV), rescale=False, resize=False, return_features=True, stages=st)
        assert feat.shape == (1, 400)
        ef = R.rel_l2(feat[0], fixture["features"][i])
        print(f"extractor vs fixture, clip {i} {tuple(fixture['clips_u8'][i].shape)} [{build}]: features rel-L2 {ef:.3e} (bound {bound:.3e})")
        worst = 0.0
        assert list(st) == R.ENDPOINTS
        for name in R.ENDPOINTS:                                                # localises a wrong layer
            e = R.rel_l2(st[name][0].double().mean(dim=(0, 1, 2)), fixture["stage_means"][name][i])
            worst = max(worst, e)
            assert e <= bound, (name, i, e)
        print(f"  worst endpoint channel mean: rel-L2 {worst:.3e}")
        assert ef <= bound


def _small_clips(n=3):
    return torch.cat([R.clip_to_bcthw(R.clip_u8(12, 32, 48, 0.4 + 0.9 * i, 7.0 + 5.0 * i, 0.5 + 0.3 * i, seed=30 + i)) for i in range(n)])


def test_deterministic_batch_and_chunk_invariant(build, net):
    from asva_amd import fvd

    clips = _small_clips().to(DEV)
    a, b = fvd.compute_fvd_video_features(clips, net), fvd.compute_fvd_video_features(clips, net)
    assert a.shape == (3, 400) and torch.equal(a, b)
    singles = torch.cat([fvd.compute_fvd_video_features(clips[i:i + 1], net) for i in range(3)])
    assert torch.equal(a, singles)
    assert torch.equal(a, fvd.compute_fvd_video_features(clips, net, chunk=2))      # a batch larger than the chunk
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])


def test_both_builds_agree_bit_for_bit(net, fixture):
    from asva_amd import _lib, fvd

    if not all(os.path.isfile(p) for p in _lib.LIB_PATHS.values()):
        pytest.skip("needs both the bf16 and the fp16 library")
    clip = R.clip_to_bcthw(fixture["clips_u8"][1]).to(DEV)                      # 17 frames: two average-pool windows

    def run():
        x = fvd.preprocess_videos(clip)
        return x.clone(), net(x).clone()

    for x, y in zip(_in_build("bf16", run), _in_build("fp16", run)):
        assert torch.equal(x, y)


def test_forward_refuses_what_the_network_cannot_take(build, net):
    with pytest.raises(ValueError, match="at least 9 frames"):
        net(torch.zeros(1, 3, 8, 224, 224, device=DEV))
    with pytest.raises(ValueError, match="7 x 7"):
        net(torch.zeros(1, 3, 12, 160, 160, device=DEV))
    with pytest.raises(NotImplementedError, match="rescale"):
        net(torch.zeros(1, 3, 12, 224, 224, device=DEV), rescale=True)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
FRAMES, FPS, SIZE, NCLIPS = 12, 6, 64, 2


def _write_dataset(root):
    """2 groundtruth videos (4 s at 6 fps, 64 x 64, 16 kHz audio) and, per groundtruth clip, one generated clip of 12 frames, in the
    pre-decoded clip container of asva_amd.data_utils"""
    rng = np.random.default_rng(0)
    names = ["beta.npz", "alpha.npz"]                                            # unsorted: the driver sorts
    (root / "gt").mkdir()
    (root / "gen").mkdir()
    for n in names:
        base = rng.integers(0, 255, (24, 8, 8, 3), dtype=np.uint8)
        frames = np.repeat(np.repeat(base, 8, 1), 8, 2)                          # (24, 64, 64, 3), blocks that change every frame
        audio = (rng.standard_normal((1, 4 * 16000)) * 0.1).astype(np.float32)
        np.savez(root / "gt" / n, frames=frames, fps=6.0, audio=audio, audio_sr=16000)
        for k in range(NCLIPS):
            gen = np.repeat(np.repeat(rng.integers(0, 255, (FRAMES, 4, 4, 3), dtype=np.uint8), 16, 1), 16, 2)
            a = (rng.standard_normal((1, 2 * 16000)) * 0.1).astype(np.float32)
            np.savez(root / "gen" / (n[:-4] + f"_clip-{k:02d}.npz"), frames=gen, fps=6.0, audio=a, audio_sr=16000)
    return names


def test_driver_fvd_equals_direct_computation(build, net, fixture, tmp_path, monkeypatch):
    from asva_amd import avsync as A
    from asva_amd import fvd
    from asva_amd.data_utils import load_av_clips_uniformly
    from avgen.evaluations.eval import evaluate_generation_results

    g = load_golden("avsync_tiny.pt")
    sd = AR.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    AR.check_draw(sd, g["probe"])
    sync = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    sync.load_state_dict(sd)
    monkeypatch.delenv(fvd.ENV_WEIGHTS, raising=False)
    names = _write_dataset(tmp_path)
    out = tmp_path / "results" / "metrics.json"
    common = dict(groundtruth_video_root=str(tmp_path / "gt"), groundtruth_video_names=list(names), groundtruth_categories=["dog", "cat"],
                  num_clips_per_video=NCLIPS, generated_video_root=str(tmp_path / "gen"), result_save_path=str(out), image_size=SIZE,
                  video_fps=FPS, video_num_frame=FRAMES, eval_fid=False, eval_clipsim=False, eval_relsync=True, eval_alignsync=False,
                  record_instance_metrics=True)
    with pytest.raises(NotImplementedError, match="eval_fvd=False"):            # no network, no $AVSD_FVD_I3D
        evaluate_generation_results(**common, models={"avsync": sync})
    without = evaluate_generation_results(**common, eval_fvd=False, models={"avsync": sync})
    res = evaluate_generation_results(**common, eval_fvd=True, models={"fvd": net, "avsync": sync})
    with open(out) as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(res))
    assert sorted(saved) == sorted(["groundtruth_video_root", "generated_video_root", "num_clips_per_video", "FVD", "RelSync_mean",
                                    "RelSync_std", "instance_metrics"])
    assert {k: v for k, v in res.items() if k != "FVD"} == without              # FVD changes no other key
    # directly: groundtruth clips in sorted order, the generated clips of each in sorted order, all frames
    gt_v, gen_v = [], []
    for n in sorted(names):
        gt_v.append(load_av_clips_uniformly(str(tmp_path / "gt" / n), FPS, FRAMES, SIZE, NCLIPS)[0])
        for k in range(NCLIPS):
            gen_v.append(load_av_clips_uniformly(str(tmp_path / "gen" / (n[:-4] + f"_clip-{k:02d}.npz")), FPS, FRAMES, SIZE, 1)[0])
    gt_v, gen_v = torch.cat(gt_v).to(DEV), torch.cat(gen_v).to(DEV)
    assert gt_v.shape == (4, FRAMES, 3, SIZE, SIZE) and gen_v.shape == gt_v.shape

    def feats(v):
        return fvd.compute_fvd_video_features(v.permute(0, 2, 1, 3, 4), net).cpu()

    want = fvd.frechet_distance(feats(gt_v), feats(gen_v)).item()
    print(f"driver [{build}]: FVD {saved['FVD']:.6f} (direct {want:.6f})")
    assert saved["FVD"] == want and saved["FVD"] > 0.0
    # the network from $AVSD_FVD_I3D (a state dict saved to a file) instead of models["fvd"]: the same value
    path = tmp_path / "i3d_state_dict.pt"
    torch.save(fixture["sd"], path)
    monkeypatch.setenv(fvd.ENV_WEIGHTS, str(path))
    assert evaluate_generation_results(**common, eval_fvd=True, models={"avsync": sync})["FVD"] == want


def test_fvd_score_tool_runs():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "fvd_score.py")], capture_output=True,
                       text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "FVD:" in r.stdout and "means nothing" in r.stdout
