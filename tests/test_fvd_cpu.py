"""FVD without a device (-m "not gpu"): the "same" padding rule, the fixture and its seeded draw, the pack-time fold and the launch
sequence driven by torch ops, the state dict, loaders, arguments, the driver's reduction and refusal, shim import paths, and the
argument checks of the two new entry points.

Bounds: the fold with torch ops against the float64 fixture within min(4 x the error of the reference module's own float32 forward,
1e-4) (tests/golden/fvd/measured.json "cpu", written by tools/gen_fvd_golden.py); everything else is compared exactly."""
import ctypes
import json
import math
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from tests import i3d_ref as R
from tests.helpers import GOLDEN, load_golden

FVD_DIR = os.path.join(GOLDEN, "fvd")


def _shapes():
    with open(os.path.join(FVD_DIR, "state_dict_shapes.json")) as f:
        return json.load(f)


def _measured():
    with open(os.path.join(FVD_DIR, "measured.json")) as f:
        return json.load(f)


def _net_bound():
    return min(4.0 * _measured()["cpu"]["f32_vs_f64_rel_l2"], 1e-4)


@pytest.fixture(scope="module")
def fixture():
    g = load_golden(os.path.join("fvd", "fvd_tiny.pt"))
    sd = R.draw_state_dict(_shapes(), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    return g


class TorchBackend:
    """the backend interface of fvd.run_network on torch ops: channels-last 5-d tensors in and out, the convolution as F.pad +
    F.conv3d on the folded, zero-padded weights, a slice write as a torch copy"""
    empty = staticmethod(lambda shape, like: torch.empty(shape, dtype=torch.float32))

    @staticmethod
    def _ret(y, out):
        y = y.permute(0, 2, 3, 4, 1)
        if out is None:
            return y.contiguous()
        out.copy_(y)
        return out

    @staticmethod
    def conv(x, layer, out=None):
        (kt, kh, kw), ci = layer.taps, layer.cin
        assert x.shape[-1] == ci
        w = layer.w[:, :kt * kh * kw * ci].view(-1, kt, kh, kw, ci).permute(0, 4, 1, 2, 3)
        y = F.relu(F.conv3d(R.pad_same(x.permute(0, 4, 1, 2, 3), layer.taps, layer.stride), w, layer.bias, layer.stride))
        return TorchBackend._ret(y, out)

    @staticmethod
    def pool(x, k, s, out=None):
        return TorchBackend._ret(F.max_pool3d(R.pad_same(x.permute(0, 4, 1, 2, 3), k, s), k, s), out)

    @staticmethod
    def mean(x, out=None):
        y = x.reshape(x.shape[0], -1, x.shape[-1]).mean(dim=1)
        if out is None:
            return y
        out.copy_(y)
        return out

    linear = staticmethod(F.linear)


# ---- the padding rule ---------------------------------------------------------------------------------------------------------------------
def test_same_padding_rule():
    from asva_amd import fvd, ops

    for size in range(1, 21):
        for k in range(1, 8):
            for s in (1, 2):
                front, back = fvd.same_pad(size, k, s)
                assert (front, back) == R.same_pad(size, k, s) == ops.same_pad(size, k, s)
                assert front == (front + back) // 2 and back - front in (0, 1)
                if size + front + back >= k:                                   # the window fits: the output is ceil(size / stride)
                    assert (size + front + back - k) // s + 1 == math.ceil(size / s), (size, k, s)
    # the cases the network meets: the stem on an even axis, the stride-2 pools, the 2 x 2 x 2 pool on t = 3
    assert fvd.same_pad(224, 7, 2) == (2, 3) and fvd.same_pad(12, 7, 2) == (2, 3) and fvd.same_pad(17, 7, 2) == (3, 3)
    assert fvd.same_pad(112, 3, 2) == (0, 1) and fvd.same_pad(3, 2, 2) == (0, 1) and fvd.same_pad(28, 3, 1) == (1, 1)


# ---- fixture, draw, state dict ------------------------------------------------------------------------------------------------------------
def test_state_dict_layout_equals_the_shapes_file():
    from asva_amd import fvd

    shapes = _shapes()
    assert {k: list(v) for k, v in fvd.state_dict_shapes().items()} == shapes
    assert shapes == R.state_dict_shapes()
    net = fvd.InceptionI3d(400, in_channels=3)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == shapes
    assert len(shapes) == 344
    assert sum(math.prod(s) for s in shapes.values()) == 12_711_881            # parameters and BatchNorm buffers
    assert fvd.InceptionI3d.VALID_ENDPOINTS[:16] == tuple(R.ENDPOINTS) and fvd.STAGE_NAMES == R.ENDPOINTS


def test_fixture_keeps_the_network_alive(fixture):
    clips = fixture["clips_u8"]
    assert [tuple(c.shape) for c in clips] == [(12, 3, 40, 56), (17, 3, 40, 56)] and all(c.dtype == torch.uint8 for c in clips)
    feats = fixture["features"]
    assert feats.shape == (2, 400) and feats.dtype == torch.float64
    assert R.rel_l2(feats[0], feats[1]) >= 0.1
    assert sorted(fixture["stage_means"]) == sorted(R.ENDPOINTS)
    cpu = _measured()["cpu"]
    assert min(cpu["nonzero_share_per_endpoint"].values()) >= 0.25 and cpu["restatement_vs_module_rel_l2"] <= 1e-12
    assert os.path.getsize(os.path.join(FVD_DIR, "fvd_tiny.pt")) < os.path.getsize(os.path.join(GOLDEN, "fid", "fid_tiny.pt"))


def test_restatement_reproduces_the_fixture(fixture):
    """clip A through the float64 restatement: the stored features (the reference module's) are those of tests/i3d_ref.py"""
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in fixture["sd"].items()}
    with torch.no_grad():
        x = R.preprocess(R.clip_to_bcthw(fixture["clips_u8"][0]))
        st = {}
        feat = R.forward(sd64, x.double(), st)
    assert x.shape == (1, 3, 12, 224, 224) and feat.shape == (1, 400)
    assert R.rel_l2(feat[0], fixture["features"][0]) < 1e-9
    # the stage shapes of the reference module for a 12-frame clip
    want = {"Conv3d_1a_7x7": (64, 6, 112, 112), "Conv3d_2c_3x3": (192, 6, 56, 56), "Mixed_3c": (480, 6, 28, 28), "Mixed_4e": (528, 3, 14, 14),
            "Mixed_4f": (832, 3, 14, 14), "MaxPool3d_5a_2x2": (832, 2, 7, 7), "Mixed_5c": (1024, 2, 7, 7)}
    for name, shape in want.items():
        assert tuple(st[name].shape[1:]) == shape, name


def test_fold_and_launch_sequence_with_torch_ops(fixture):
    """the pack-time fold (BatchNorm into weights, zero-padded activation widths, b1a and b2a stacked) and the launch sequence with its
    channel slices, driven by torch ops instead of the device library: float32 against the float64 fixture, clip A"""
    from asva_amd import fvd

    bound = _net_bound()
    pk = fvd.fold_network(fixture["sd"])
    by_name = {n: b for (n, _, _), b in zip(fvd.MIXED, pk.blocks)}
    assert pk.stem[0].cin == 3 and pk.stem[0].w.shape == (64, 1032)
    assert by_name["Mixed_3b"].red.cout == 96 + 32 and by_name["Mixed_3b"].b2b.cin == 32 and by_name["Mixed_3b"].split == 96
    assert by_name["Mixed_4c"].red.cout == 128 + 32 and by_name["Mixed_4c"].b1b.cin == 128
    assert by_name["Mixed_4e"].red.cout == 160 + 32 and by_name["Mixed_4e"].b3b.cout == 80 and by_name["Mixed_4e"].width == 528
    assert by_name["Mixed_4f"].b0.cin == 544 and by_name["Mixed_5c"].red.cout == 192 + 64
    assert not bool(by_name["Mixed_4e"].b3b.w[64:].any()) and not bool(by_name["Mixed_4e"].b3b.bias[64:].any())
    for b in pk.blocks:                                                         # every consumer takes the float4 loader
        for layer in (b.b0, b.red, b.b1b, b.b2b, b.b3b):
            assert layer.cin % 32 == 0 and layer.w.shape[1] % 4 == 0
    with torch.no_grad():
        x = R.preprocess(R.clip_to_bcthw(fixture["clips_u8"][0]))
        st = {}
        feat = fvd.run_network(pk, x.permute(0, 2, 3, 4, 1).contiguous(), be=TorchBackend, stages=st)
    e = R.rel_l2(feat[0], fixture["features"][0])
    print(f"fold with torch ops: features rel-L2 {e:.3e} (bound {bound:.3e})")
    assert feat.shape == (1, 400) and e <= bound
    assert list(st) == fvd.STAGE_NAMES
    widths = {"Mixed_4e": 528, "Mixed_4f": 832, "Mixed_5c": 1024}
    for name, y in st.items():
        e = R.rel_l2(y[0].double().mean(dim=(0, 1, 2)), fixture["stage_means"][name][0])
        assert e <= bound, (name, e)
        assert y.shape[-1] == widths.get(name, y.shape[-1])


def test_state_dict_loading_and_repacking(fixture):
    from asva_amd import fvd

    net = fvd.InceptionI3d()
    net.load_state_dict(fixture["sd"])
    for k, v in fixture["sd"].items():
        assert torch.equal(net.state_dict()[k], v)
    bad = dict(fixture["sd"])
    del bad["Mixed_4c.b2a.conv3d.weight"]
    with pytest.raises(KeyError, match="Mixed_4c.b2a.conv3d.weight"):
        fvd.InceptionI3d().load_state_dict(bad)
    extra = dict(fixture["sd"], **{"Mixed_9z.b0.conv3d.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="unexpected"):
        fvd.InceptionI3d().load_state_dict(extra)
    wrong = dict(fixture["sd"], **{"Conv3d_2b_1x1.conv3d.weight": torch.zeros(64, 64, 3, 1, 1)})
    with pytest.raises(ValueError, match="Conv3d_2b_1x1.conv3d.weight"):
        fvd.InceptionI3d().load_state_dict(wrong)
    epoch = net._epoch
    net.load_state_dict(fixture["sd"])
    assert net._epoch > epoch                                                   # a cached pack is stale after load_state_dict
    # bn_eps enters the fold
    a, b = fvd.fold_network(fixture["sd"], 1e-5), fvd.fold_network(fixture["sd"], 1e-3)
    assert not torch.equal(a.stem[0].w, b.stem[0].w)


# ---- loaders and arguments ----------------------------------------------------------------------------------------------------------------
def test_loader_needs_weights_and_never_opens_a_socket(monkeypatch, tmp_path, fixture):
    from asva_amd import fvd

    def no_socket(*a, **k):
        raise AssertionError("the loader tried to open a socket")

    monkeypatch.setattr(socket, "socket", no_socket)
    monkeypatch.delenv(fvd.ENV_WEIGHTS, raising=False)
    with pytest.raises(FileNotFoundError) as e:
        fvd.load_i3d_pretrained()
    assert "weights" in str(e.value) and fvd.ENV_WEIGHTS in str(e.value)
    monkeypatch.setenv(fvd.ENV_WEIGHTS, str(tmp_path / "missing.pt"))
    with pytest.raises(FileNotFoundError, match="missing.pt"):
        fvd.load_i3d_pretrained()
    path = tmp_path / "i3d_state_dict.pt"
    torch.save(fixture["sd"], path)
    monkeypatch.setenv(fvd.ENV_WEIGHTS, str(path))
    a = fvd.load_i3d_pretrained()
    b = fvd.load_i3d_pretrained(weights=fixture["sd"], bn_eps=1e-3)
    assert a.bn_eps == fvd.BN_EPS == 1e-5 and b.bn_eps == 1e-3 and a.num_classes == 400
    for k, v in fixture["sd"].items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v)


def test_loader_opens_a_torchscript_archive_for_its_state_dict(tmp_path, fixture):
    """a scripted module that holds the state dict's tensors under the module's names: only state_dict() of the archive is used, and
    an archive defaults to the TensorFlow epsilon"""
    from asva_amd import fvd

    class Holder(torch.nn.Module):
        def forward(self, x):
            return x

    root = Holder()
    for key, v in fixture["sd"].items():
        mod, parts = root, key.split(".")
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, Holder())
            mod = mod._modules[p]
        mod.register_buffer(parts[-1], v.clone())
    path = tmp_path / "i3d_torchscript.pt"
    torch.jit.save(torch.jit.script(root), str(path))
    net = fvd.load_i3d_pretrained(weights=str(path))
    assert net.bn_eps == fvd.ARCHIVE_BN_EPS == 1e-3
    for k, v in fixture["sd"].items():
        assert torch.equal(net.state_dict()[k], v)
    assert fvd.load_i3d_pretrained(weights=str(path), bn_eps=1e-5).bn_eps == 1e-5


def test_unsupported_arguments_raise(monkeypatch):
    from asva_amd import fvd
    from asva_amd.evaluation import FVD_MESSAGE, evaluate_generation_results

    with pytest.raises(NotImplementedError, match="spatial_squeeze"):
        fvd.InceptionI3d(spatial_squeeze=False)
    with pytest.raises(NotImplementedError, match="final_endpoint"):
        fvd.InceptionI3d(final_endpoint="Mixed_4f")
    with pytest.raises(ValueError, match="Unknown final endpoint"):
        fvd.InceptionI3d(final_endpoint="Mixed_9z")
    with pytest.raises(ValueError, match="float32"):
        fvd.InceptionI3d().to(dtype=torch.float16)
    assert fvd.InceptionI3d().to(dtype=torch.float32) is not None
    net = fvd.InceptionI3d()
    with pytest.raises(NotImplementedError, match="rescale"):
        net(torch.zeros(1, 3, 12, 224, 224), rescale=True)
    with pytest.raises(NotImplementedError, match="resize"):
        net(torch.zeros(1, 3, 12, 224, 224), resize=True)
    with pytest.raises(ValueError, match="at least 9 frames"):
        net(torch.zeros(1, 3, 8, 224, 224))
    with pytest.raises(ValueError, match="7 x 7"):
        net(torch.zeros(1, 3, 12, 160, 160))
    with pytest.raises(ValueError, match="7 x 7"):
        net(torch.zeros(1, 3, 12, 224, 225))
    with pytest.raises(ValueError):
        fvd.compute_fvd_video_features(torch.zeros(1, 3, 12, 32, 32), net, chunk=0)
    # eval_fvd=True without a network and without $AVSD_FVD_I3D is refused before any file is read: the roots do not exist
    monkeypatch.delenv(fvd.ENV_WEIGHTS, raising=False)
    assert "eval_fvd=False" in FVD_MESSAGE and fvd.ENV_WEIGHTS in FVD_MESSAGE and "models" in FVD_MESSAGE
    with pytest.raises(NotImplementedError, match="eval_fvd=False"):
        evaluate_generation_results("/nonexistent/gt", ["a.mp4"], ["dog"], 1, "/nonexistent/gen", "/nonexistent/out.json", 64)
    with pytest.raises(NotImplementedError, match="eval_fvd=False"):
        evaluate_generation_results("/nonexistent/gt", ["a.mp4"], ["dog"], 1, "/nonexistent/gen", "/nonexistent/out.json", 64, models={"fid": net})


def test_reduction_adds_fvd_and_leaves_the_other_keys(fixture):
    from asva_amd.evaluation import reduce_metrics
    from asva_amd.fid import frechet_distance

    g = torch.Generator().manual_seed(5)
    gt = [torch.randn(2, 16, generator=g) for _ in range(3)]
    gen = [torch.randn(1, 16, generator=g) + 0.2 for _ in range(6)]
    gt_s, gen_s = [torch.randn(2, generator=g) for _ in range(3)], [torch.randn(1, generator=g) for _ in range(6)]
    base = reduce_metrics(groundtruth_avsync_scores=gt_s, generated_avsync_scores=gen_s)
    got = reduce_metrics(groundtruth_avsync_scores=gt_s, generated_avsync_scores=gen_s, groundtruth_fvd_features=gt, generated_fvd_features=gen)
    assert sorted(got) == ["FVD", "RelSync_mean", "RelSync_std"]
    assert got["FVD"] == frechet_distance(torch.cat(gt), torch.cat(gen)).item() and got["FVD"] > 0.0
    assert {k: v for k, v in got.items() if k != "FVD"} == base
    with pytest.raises(TypeError):
        reduce_metrics(None, None, None, None, None, None, None, None, None, gt, gen)      # the new arguments are keywords


def test_shim_import_paths_resolve():
    import asva_amd.fvd as fvd
    from avgen.evaluations.fvd import compute_fvd_video_features
    from avgen.evaluations.fvd.compute_fvd import preprocess_videos
    from avgen.evaluations.models.download import load_i3d_pretrained
    from avgen.evaluations.models.pytorch_i3d import InceptionI3d

    assert compute_fvd_video_features is fvd.compute_fvd_video_features and preprocess_videos is fvd.preprocess_videos
    assert load_i3d_pretrained is fvd.load_i3d_pretrained and InceptionI3d is fvd.InceptionI3d


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def conv(to=1, ho=2, wo=2, ldx=32, ldy=32, cin=32, cout=32, loader=0, ldw=None, x=p):
        return h.avsd_conv3d_same_f32(x, ldx, p, None, p, ldy, 1, 2, 4, 4, cin, to, ho, wo, cout, 3, 3, 3, 2, 2, 2,
                                      27 * cin if ldw is None else ldw, 0, loader, None)

    assert conv(to=2) == -1 and b"ceil(input / stride)" in h.avsd_last_error()
    assert conv(ho=1) == -1 and b"ceil(input / stride)" in h.avsd_last_error()
    assert conv(ldx=31) == -1 and b"ldx" in h.avsd_last_error()
    assert conv(ldy=31) == -1 and b"ldy" in h.avsd_last_error()
    assert conv(loader=4) == -1 and b"loader must be" in h.avsd_last_error()
    assert conv(loader=2, cin=3, ldx=3) == -1 and b"loader 2" in h.avsd_last_error()
    assert conv(loader=3, ldx=64) == -1 and b"loader 3" in h.avsd_last_error()
    assert conv(ldw=27 * 32 - 1) == -1 and b"ldw" in h.avsd_last_error()
    assert conv(x=None) == -1 and b"null" in h.avsd_last_error()

    def pool(k=(3, 3, 3), s=(2, 2, 2), out=(1, 2, 2), c=8, ldx=8, ldy=8):
        return h.avsd_maxpool3d_same_f32(p, ldx, p, ldy, 1, 2, 4, 4, c, *out, *k, *s, None)

    assert pool(out=(1, 2, 1)) == -1 and b"ceil(input / stride)" in h.avsd_last_error()
    assert pool(k=(4, 3, 3)) == -1 and b"windows must be 1 .. 3" in h.avsd_last_error()
    assert pool(s=(3, 2, 2), out=(1, 2, 2)) == -1 and b"strides must be 1 .. 2" in h.avsd_last_error()
    assert pool(c=6) == -1 and b"multiple of 4" in h.avsd_last_error()
    assert pool(ldx=4) == -1 and b"ldx" in h.avsd_last_error()
    assert pool(ldy=10) == -1 and b"ldy" in h.avsd_last_error()
