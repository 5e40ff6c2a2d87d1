"""AVSync scorer without a GPU (-m "not gpu"): the state-dict surface, the restatement tests/avsync_ref.py against the fixture the
reference's own modules wrote (tools/gen_avsync_golden.py), the BatchNorm fold and weight re-layout of pack() applied with plain
torch ops, the host-built resize taps, the RelSync contract, and the argument checks of the four entry points.

Bounds: both sides of the restatement check are fp32 CPU torch -> rel-L2 < 1e-6 (the reference's own fp32 result lies 0.7e-7 -
2.1e-7 from its float64 run: avsync_tiny.pt "reference_fp32_error").  Resize taps: 4 x the deviation measured when the fixture was
written (tests/golden/avsync_measured.json; summation order only), and in any case below 1e-5 absolute on values of order 1.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import avsync_ref as R
from tests.helpers import GOLDEN, load_golden, load_shapes


@pytest.fixture(scope="module")
def fixture():
    g = load_golden("avsync_tiny.pt")
    sd = R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    g["video"] = R.normalize_clip(R.u8_to_unit(g["video_u8"]))
    return g


def _classifier():
    from asva_amd import avsync as A

    return A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()


def test_state_dict_surface():
    shapes = load_shapes("avsync_state_dict_shapes.json")
    sd = _classifier().state_dict()
    assert len(shapes) == 261
    assert {k: list(v.shape) for k, v in sd.items()} == shapes
    assert list(sd) == list(shapes)                      # the same order as the reference's modules


def test_load_avsync_model_round_trip(tmp_path, fixture):
    from asva_amd import avsync as A

    sd = fixture["sd"]
    for sub, cls, cfg in (("audio_encoder", "AudioConv2DNet", {"pretrained": False}), ("video_encoder", "VideoR2Plus1DNet", {"pretrained": False}),
                          ("head", "FCHead", {"dim": 512, "out_dim": 1, "dropout": 0.0})):
        d = tmp_path / sub
        d.mkdir()
        (d / "config.json").write_text(json.dumps({"_class_name": cls, "_diffusers_version": "0.29.2", **cfg}))
        torch.save(R._sub(sd, sub + "."), d / "diffusion_pytorch_model.bin")
    net = A.load_avsync_model(str(tmp_path))
    assert not net.training and not any(p.requires_grad for p in net.parameters())
    got = net.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())
    net.video_encoder.save_pretrained(str(tmp_path / "again"))
    again = A.VideoR2Plus1DNet.from_pretrained(str(tmp_path / "again"), use_safetensors=False)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in net.video_encoder.state_dict().items())
    with pytest.raises(FileNotFoundError):
        A.FCHead.from_pretrained(str(tmp_path / "audio_encoder" / ".."), use_safetensors=False)


def test_reference_import_paths():
    from asva_amd import avsync as A
    from avgen.evaluations.avsync.compute_avsync import compute_avsync_scores, compute_relsync, compute_sync_metrics_on_av, preprocess_videos
    from avsync.models.audio import AudioConv2DNet
    from avsync.models.avsync_classifier import AVSyncClassifier, load_avsync_model
    from avsync.models.head import FCHead
    from avsync.models.video import VideoR2Plus1DNet

    assert AVSyncClassifier is A.AVSyncClassifier and load_avsync_model is A.load_avsync_model and compute_relsync is A.compute_relsync
    assert (AudioConv2DNet, VideoR2Plus1DNet, FCHead) == (A.AudioConv2DNet, A.VideoR2Plus1DNet, A.FCHead)
    assert all(callable(f) for f in (compute_avsync_scores, compute_sync_metrics_on_av, preprocess_videos))


def test_restatement_against_the_reference_fixture(fixture):
    sd = fixture["sd"]
    a_st, v_st = [], []
    with torch.no_grad():
        a = R.audio_forward(R._sub(sd, "audio_encoder."), fixture["audio"], a_st)
        v = R.video_forward(R._sub(sd, "video_encoder."), fixture["video"], v_st)
        scores = torch.stack([torch.stack([R.classifier_forward(sd, fixture["audio"][i:i + 1], fixture["video"][j:j + 1])[0] for j in range(2)])
                              for i in range(2)])
    assert R.rel_l2(a, fixture["audio_emb"]) < 1e-6 and R.rel_l2(v, fixture["video_emb"]) < 1e-6
    for prefix, names, st in (("a.", ["conv1", "block1", "block2", "block3", "block4"], a_st), ("v.", ["conv1", "conv2x", "conv3x", "conv4x", "conv5x"], v_st)):
        for nm, y in zip(names, st):
            assert R.rel_l2(y[0].reshape(y.shape[1], -1).mean(1), fixture["stage_means"][prefix + nm]) < 1e-6, prefix + nm
    assert R.rel_l2(scores, fixture["scores"]) < 1e-6
    own = torch.stack([scores[0, 0], scores[1, 1]])
    assert (R.relsync(torch.stack([scores[1, 0], scores[0, 1]]), own) - fixture["relsync_ref_audio"]).abs().max() < 1e-6
    assert (R.relsync(torch.stack([scores[0, 1], scores[1, 0]]), own) - fixture["relsync_ref_video"]).abs().max() < 1e-6


class _TorchBackend:
    """what the device library computes from the packed layers, with plain torch ops: undoes the [cout][taps][cin] layout and calls
    F.conv3d; epilogue bias + rscale * res, ReLU"""

    @staticmethod
    def conv(x, layer, res=None):
        kt, kh, kw = layer.taps
        k = kt * kh * kw * layer.cin
        assert layer.w.shape == (layer.cout, (k + 3) // 4 * 4) and layer.w.dtype == torch.float32 and not layer.w[:, k:].any()
        w = layer.w[:, :k].reshape(layer.cout, kt, kh, kw, layer.cin).permute(0, 4, 1, 2, 3)
        y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, layer.bias, layer.stride, layer.pad).permute(0, 2, 3, 4, 1)
        if res is not None:
            y = y + (layer.rscale if layer.rscale is not None else 1.0) * res
        return (y.relu() if layer.relu else y).contiguous()

    @staticmethod
    def maxpool(x):
        return F.max_pool3d(x.permute(0, 4, 1, 2, 3), (1, 3, 3), (1, 2, 2), (0, 1, 1)).permute(0, 2, 3, 4, 1).contiguous()

    @staticmethod
    def mean(x):
        return x.reshape(x.shape[0], -1, x.shape[-1]).mean(1)


def test_batchnorm_fold_and_relayout_reproduce_the_restatement(fixture):
    from asva_amd import avsync as A

    net = _classifier()
    net.load_state_dict(fixture["sd"])
    with torch.no_grad():
        a = A.run_audio(A.fold_audio(net.audio_encoder), net._audio_cl(fixture["audio"]), _TorchBackend)
        v = A.run_video(A.fold_video(net.video_encoder), net._video_cl(fixture["video"]), _TorchBackend)
        s = A.run_head(A.fold_head(net.head), a, v, _TorchBackend)[:, 0]
    assert R.rel_l2(a, fixture["audio_emb"]) < 1e-6 and R.rel_l2(v, fixture["video_emb"]) < 1e-6
    assert R.rel_l2(s, torch.stack([fixture["scores"][0, 0], fixture["scores"][1, 1]])) < 1e-6
    # the identity residual is scaled in the epilogue, the projected one inside its weights
    fv = A.fold_video(net.video_encoder)
    assert fv.stages[0][0].res is None and fv.stages[0][0].tmp2.rscale is not None
    assert fv.stages[1][0].res is not None and fv.stages[1][0].tmp2.rscale is None and fv.stages[1][0].res.stride == (2, 2, 2)


def test_pack_is_cached_and_follows_load_state_dict(fixture):
    from asva_amd import avsync as A, ops

    net = _classifier()
    old = getattr(ops, "EMULATED", False)
    ops.EMULATED = True                                  # lets pack() target the CPU (the seam tests/emu_ops.py uses)
    try:
        pk = net.pack("cpu")
        assert net.pack("cpu") is pk and pk.blob.dtype == torch.uint8 and pk.video.conv1.w.dtype == torch.float32
        assert pk.video.conv1.w.untyped_storage().data_ptr() == pk.blob.untyped_storage().data_ptr()       # one blob
        net.load_state_dict(fixture["sd"])
        pk2 = net.pack("cpu")
        assert pk2 is not pk and torch.equal(pk2.head[0].w, A.fold_head(net.head)[0].w)
        net.video_encoder.load_state_dict(net.video_encoder.state_dict())
        assert net.pack("cpu") is not pk2                # a sub-network loaded on its own repacks too
        net.train()
        net._packed = None
        with pytest.raises(RuntimeError, match="eval"):
            net.pack("cpu")
    finally:
        ops.EMULATED = old


@pytest.mark.parametrize("name", ["avsync_preprocess.pt", "avsync_preprocess_128x256.pt"])
def test_resize_tables_reproduce_the_fixture(name):
    from asva_amd import avsync as A

    g = load_golden(name)
    x = R.u8_to_unit(g["frames_u8"])
    mats = []
    for n in x.shape[2:]:
        start, count, weight = A.resize_tables(n, 224)
        assert weight.shape[1] <= n and (start >= 0).all() and (start + count <= n).all() and (count <= weight.shape[1]).all()
        m = torch.zeros(224, n)
        for i in range(224):
            m[i, start[i]:start[i] + count[i]] = torch.from_numpy(weight[i, :count[i]])
            assert not weight[i, count[i]:].any()
        mats.append(m)
    y = torch.einsum("oh,nchw->ncow", mats[0], torch.einsum("pw,nchw->nchp", mats[1], x))
    y = (y - torch.tensor(A.CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.CLIP_STD).view(1, 3, 1, 1)
    err = (y - g["out"]).abs().max().item()
    with open(os.path.join(GOLDEN, "avsync_measured.json")) as f:
        measured = json.load(f)["cpu"]["resize_tables_max_abs"]
    print(f"resize tables vs F.interpolate(bicubic, antialias) {name}: max abs {err:.3e} (measured {measured:.3e})")
    assert err <= min(4.0 * measured, 1e-5)


def test_relsync_contract():
    from asva_amd import avsync as A

    a, v = torch.zeros(1, 1, 128, 204), torch.zeros(1, 3, 12, 8, 8)
    with pytest.raises(ValueError, match="either ref_audios or ref_videos"):
        A.compute_relsync(a, v, None)
    with pytest.raises(ValueError, match="either ref_audios or ref_videos"):
        A.compute_relsync(a, v, None, ref_audios=a, ref_videos=v)
    ref, own = torch.tensor([0.0, 1.0, -2.0]), torch.tensor([0.0, 3.0, -2.5])
    want = torch.tensor([0.5, 1.0 / (1.0 + 2.718281828459045 ** -2.0), 1.0 / (1.0 + 2.718281828459045 ** 0.5)])
    assert torch.allclose(A.relsync_from_scores(ref, own), want, atol=1e-7)
    wave, clip = torch.zeros(1, 32000), torch.zeros(3, 12, 8, 8)
    with pytest.raises(NotImplementedError, match="ImageBind"):
        A.compute_sync_metrics_on_av(wave, 16000, clip, ref_video=clip, metric="alignsync")
    with pytest.raises(ValueError, match="16000"):
        A.compute_sync_metrics_on_av(wave, 22050, clip, metric="avsync_score")
    with pytest.raises(ValueError, match="relsync"):
        A.compute_sync_metrics_on_av(wave, 16000, clip, metric="relsync")


def test_entry_points_refuse_bad_arguments_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    p = 4096                                             # never dereferenced: every call below is refused before any launch
    conv = lambda *a: h.avsd_convnd_f32(*a)              # noqa: E731
    geom = [1, 4, 8, 8, 64, 4, 8, 8, 64, 1, 3, 3, 1, 1, 1, 0, 1, 1, 576, 1]
    assert conv(None, p, None, None, None, p, *geom, None) == -1 and b"null" in h.avsd_last_error()
    assert conv(p, p, None, None, None, p, *(geom[:6] + [7] + geom[7:]), None) == -1 and b"does not follow" in h.avsd_last_error()
    assert conv(p, p, None, None, None, p, *(geom[:4] + [0] + geom[5:]), None) == -1 and b"positive" in h.avsd_last_error()
    assert conv(p, p, None, None, None, p, *(geom[:18] + [572] + geom[19:]), None) == -1 and b"ldw" in h.avsd_last_error()
    assert conv(p, p, None, None, p, p, *geom, None) == -1 and b"rscale" in h.avsd_last_error()
    assert h.avsd_maxpool_hw_f32(p, None, 1, 8, 8, 64, 4, 4, None) == -1 and b"null" in h.avsd_last_error()
    assert h.avsd_maxpool_hw_f32(p, p, 1, 8, 8, 64, 3, 4, None) == -1 and b"does not follow" in h.avsd_last_error()
    assert h.avsd_maxpool_hw_f32(p, p, 1, 8, 8, 6, 4, 4, None) == -1 and b"multiple of 4" in h.avsd_last_error()
    assert h.avsd_mean_rows_f32(p, p, 2, 0, 64, None) == -1 and b"positive" in h.avsd_last_error()
    assert h.avsd_mean_rows_f32(None, p, 2, 4, 64, None) == -1 and b"null" in h.avsd_last_error()
    rs = lambda crop, taps, x=p: h.avsd_resize_aa_normalize_f32(x, p, p, 1, 256, 256, 224, 224, p, p, p, taps, p, p, p, 7, crop,  # noqa: E731
                                                                0.5, 0.5, 0.5, 0.25, 0.25, 0.25, None)
    assert rs(224, 7, None) == -1 and b"null" in h.avsd_last_error()
    assert rs(200, 7) == -1 and b"centre crop" in h.avsd_last_error()
    assert rs(224, 0) == -1 and b"positive" in h.avsd_last_error()
