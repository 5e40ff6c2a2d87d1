"""FID without a device (-m "not gpu"): the Fréchet distance against the reference's own formula, the reduction function of the
evaluation driver against a literal restatement of eval.py:203-247, the fixture and its seeded draw, the pack-time fold driven by torch
ops, loaders, arguments and shim import paths.

Bounds: the Fréchet distance within 1e-6 (tr S1 + tr S2 + |mu1 - mu2|^2) of numpy + scipy.linalg.sqrtm (measured: at most 7.9e-9,
tests/golden/fid/measured.json "frechet"); identical sets give |FD| < 1e-6 in both; the reduction is compared exactly."""
import json
import os
import socket
import sys

import pytest
import torch

from tests import inception_ref as R
from tests.helpers import GOLDEN, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))

FID_DIR = os.path.join(GOLDEN, "fid")


def _shapes():
    with open(os.path.join(FID_DIR, "state_dict_shapes.json")) as f:
        return json.load(f)


def _measured():
    with open(os.path.join(FID_DIR, "measured.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    g = load_golden(os.path.join("fid", "fid_tiny.pt"))
    sd = R.draw_state_dict(_shapes(), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    return g


# ---- Fréchet distance -----------------------------------------------------------------------------------------------------------------
FD_SIZES = [(200, 160, 32), (64, 48, 32), (500, 400, 128), (20, 24, 32), (96, 96, 128)]


@pytest.mark.parametrize("n1,n2,d", FD_SIZES)
def test_frechet_distance_against_the_reference_formula(n1, n2, d):
    import gen_fid_golden as G
    from asva_amd.fid import frechet_distance

    x1, x2 = G.fd_features(n1, d, 11 * d + n1), G.fd_features(n2, d, 13 * d + n2, shift=0.05)
    ours = frechet_distance(x1, x2)
    assert ours.dtype == torch.float64 and ours.dim() == 0 and isinstance(ours.item(), float)
    ref, scale, fallback, imag = G.fd_reference(x1.clone(), x2.clone())
    print(f"frechet {n1}x{n2}x{d}: ours {ours.item():.12g}, reference {ref:.12g}, |d| / scale {abs(ours.item() - ref) / scale:.3e}, "
          f"reference fallback {fallback}, max imaginary part {imag:.2e}")
    assert not fallback and imag <= 1e-3                      # the comparison is against the reference's main branch
    assert abs(ours.item() - ref) <= 1e-6 * scale
    same, same_ref = frechet_distance(x1, x1.clone()).item(), G.fd_reference(x1.clone(), x1.clone())[0]
    print(f"  identical sets: ours {same:.3e}, reference {same_ref:.3e}")
    assert abs(same) < 1e-6 and abs(same_ref) < 1e-6
    rec = _measured()["frechet"][f"{n1}x{n2}x{d}"]
    assert abs(rec["ours"] - ours.item()) <= 1e-9 * scale     # the recorded figures are those of this code


def test_frechet_distance_refuses_bad_inputs():
    from asva_amd.fid import frechet_distance

    with pytest.raises(ValueError, match="two samples"):
        frechet_distance(torch.randn(1, 8), torch.randn(5, 8))
    with pytest.raises(ValueError, match="two samples"):
        frechet_distance(torch.randn(5, 8), torch.randn(1, 8))
    with pytest.raises(ValueError, match="widths"):
        frechet_distance(torch.randn(5, 8), torch.randn(5, 9))
    x = torch.randn(6, 4)
    keep = x.clone()
    frechet_distance(x, x)
    assert torch.equal(x, keep)                                # the inputs are not centred in place


# ---- the reduction function of the driver -----------------------------------------------------------------------------------------------
def _restated_reduction(gt_fid, gen_fid, gen_ias, gen_its, gt_scores, gen_scores, gt_first, gen_pred):
    """eval.py:203-247, literally (FVD left out), on lists of per-video / per-clip tensors"""
    from asva_amd.fid import frechet_distance

    result_dict = {}
    groundtruth_fid_features = torch.cat(gt_fid)[:, 1:].flatten(end_dim=1)
    generated_fid_features = torch.cat(gen_fid)[:, 1:].flatten(end_dim=1)
    fid_score = frechet_distance(groundtruth_fid_features, generated_fid_features)
    result_dict["FID"] = fid_score.item()
    generated_ias = torch.cat(gen_ias)
    generated_its = torch.cat(gen_its)
    result_dict.update({"IA_mean": generated_ias.mean().item(), "IA_std": generated_ias.std().item(),
                        "IT_mean": generated_its.mean().item(), "IT_std": generated_its.std().item()})
    groundtruth_avsync_scores = torch.cat(gt_scores)
    generated_avsync_scores = torch.cat(gen_scores)
    generated_relsync_scores = torch.exp(generated_avsync_scores) / (torch.exp(groundtruth_avsync_scores) + torch.exp(generated_avsync_scores))
    result_dict.update({"RelSync_mean": generated_relsync_scores.mean().item(), "RelSync_std": generated_relsync_scores.std().item()})
    groundtruth_first_frame_ia_sims = torch.cat(gt_first)
    generated_pred_frame_ia_sims = torch.cat(gen_pred)
    generated_align_probs = (torch.exp(generated_pred_frame_ia_sims)
                             / (torch.exp(groundtruth_first_frame_ia_sims) + torch.exp(generated_pred_frame_ia_sims))).mean(dim=1)
    generated_alignsync_scores = generated_align_probs * generated_relsync_scores
    result_dict.update({"AlignSync_mean": generated_alignsync_scores.mean().item(), "AlignSync_std": generated_alignsync_scores.std().item()})
    return result_dict, generated_ias, generated_its, generated_relsync_scores, generated_alignsync_scores


def test_reduction_matches_the_restated_steps_4_and_5():
    from asva_amd.evaluation import reduce_metrics

    g = torch.Generator().manual_seed(3)
    videos, clips, frames, c = 3, 2, 5, 16
    gt_fid = [torch.randn(clips, frames, c, generator=g).relu() for _ in range(videos)]
    gen_fid = [torch.randn(1, frames, c, generator=g).relu() + 0.1 for _ in range(videos * clips)]
    gen_pred = [0.3 * torch.randn(1, frames - 1, generator=g) for _ in range(videos * clips)]
    gen_ias = [p.mean(dim=1) for p in gen_pred]
    gen_its = [0.3 * torch.randn(1, generator=g) for _ in range(videos * clips)]
    gt_scores = [torch.randn(clips, generator=g) for _ in range(videos)]
    gen_scores = [torch.randn(1, generator=g) for _ in range(videos * clips)]
    gt_first = [0.3 * torch.randn(clips, 1, generator=g) for _ in range(videos)]
    names = [f"v{i}_clip-{k:02d}.mp4" for i in range(videos) for k in range(clips)]
    want, ias, its, rel, align = _restated_reduction(gt_fid, gen_fid, gen_ias, gen_its, gt_scores, gen_scores, gt_first, gen_pred)
    got = reduce_metrics(gt_fid, gen_fid, gen_ias, gen_its, gt_scores, gen_scores, gt_first, gen_pred, generated_video_names=names)
    keys = ["FID", "IA_mean", "IA_std", "IT_mean", "IT_std", "RelSync_mean", "RelSync_std", "AlignSync_mean", "AlignSync_std"]
    assert sorted(k for k in got if k != "instance_metrics") == sorted(keys)
    for k in keys:
        assert got[k] == want[k], (k, got[k], want[k])
    inst = got["instance_metrics"]
    assert list(inst) == names
    for i, n in enumerate(names):
        # "IT" holds the IT value: the reference's record repeats IA there (eval.py:269)
        assert inst[n] == {"IA": ias[i].item(), "IT": its[i].item(), "RelSync": rel[i].item(), "AlignSync": align[i].item()}
    assert any(inst[n]["IT"] != inst[n]["IA"] for n in names)
    # a subset of the metrics: only their keys
    part = reduce_metrics(groundtruth_avsync_scores=gt_scores, generated_avsync_scores=gen_scores)
    assert sorted(part) == ["RelSync_mean", "RelSync_std"] and part["RelSync_mean"] == want["RelSync_mean"]


# ---- fixture, draw, fold ------------------------------------------------------------------------------------------------------------------
def test_state_dict_layout_equals_the_shapes_file():
    from asva_amd import fid

    shapes = _shapes()
    assert {k: list(v) for k, v in fid.state_dict_shapes().items()} == shapes
    assert shapes == R.state_dict_shapes()
    net = fid.InceptionV3((3,))
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == shapes
    assert sum(int(torch.tensor(s).prod()) if s else 1 for k, s in shapes.items() if k.endswith(("conv.weight", "fc.weight"))) > 23_000_000


def test_fixture_keeps_the_network_alive(fixture):
    imgs = fixture["images_u8"]
    assert [tuple(i.shape) for i in imgs] == [(3, 256, 256), (3, 128, 200), (3, 75, 91)] and all(i.dtype == torch.uint8 for i in imgs)
    feats = fixture["features"]
    assert feats.shape == (3, 2048) and feats.dtype == torch.float64 and fixture["logits"].shape == (3, 1008)
    assert all(int((f != 0).sum()) >= 1024 for f in feats)
    for i in range(3):
        for j in range(i):
            assert not torch.equal(feats[i], feats[j])
    assert sorted(fixture["stage_means"]) == sorted(R.STAGES)


def test_restatement_reproduces_the_fixture(fixture):
    """the smallest image through the float64 restatement: the stored features are those of tests/inception_ref.py"""
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in fixture["sd"].items()}
    with torch.no_grad():
        x = R.preprocess(R.u8_to_unit(fixture["images_u8"][2])[None])
        feat, logits = R.forward(sd64, x.double())
    assert R.rel_l2(feat[0], fixture["features"][2]) < 1e-6 and R.rel_l2(logits[0], fixture["logits"][2]) < 1e-6


def test_fold_and_launch_sequence_with_torch_ops(fixture):
    """the pack-time fold (BatchNorm into weights, zero-padded 48 / 80 channel activations, stacked 1 x 1 convolutions) and the launch
    sequence with its channel slices, driven by torch ops instead of the device library: float32 against the float64 fixture.
    Bound: 4 x the error of torch's own float32 forward, capped at 1e-4 (tests/golden/fid/measured.json "cpu")."""
    import fid_bench
    from asva_amd import fid

    bound = min(4.0 * _measured()["cpu"]["f32_vs_f64_rel_l2"], 1e-4)
    pk = fid.fold_network(fixture["sd"])
    assert pk.stem[3].cout == 96 and pk.stem[4].cin == 96 and pk.blocks[0].b5.cin == 64 and pk.blocks[0].red.cout == 128
    assert all(not bool(pk.stem[3].w[80:].any()) and not bool(pk.stem[3].bias[80:].any()) for _ in (0,))
    with torch.no_grad():
        x = R.preprocess(R.u8_to_unit(fixture["images_u8"][2])[None])
        st = {}
        outs = fid.run_network(pk, x.permute(0, 2, 3, 1).contiguous().unsqueeze(1), 4, be=fid_bench._Torch, stages=st)
    ef, el = R.rel_l2(outs[3][0], fixture["features"][2]), R.rel_l2(outs[4][0], fixture["logits"][2])
    print(f"fold with torch ops: features rel-L2 {ef:.3e}, logits {el:.3e} (bound {bound:.3e})")
    assert ef <= bound and el <= bound
    assert list(st) == fid.STAGE_NAMES == R.STAGES
    for name, y in st.items():
        e = R.rel_l2(y[0, 0].double().mean(dim=(0, 1)), fixture["stage_means"][name][2])
        assert e <= bound, (name, e)
    assert outs[0].shape[-1] == 64 and outs[1].shape[-1] == 192 and outs[2].shape[-1] == 768


# ---- loaders and arguments ------------------------------------------------------------------------------------------------------------------
def test_loader_needs_weights_and_never_opens_a_socket(monkeypatch, tmp_path, fixture):
    from asva_amd import fid

    def no_socket(*a, **k):
        raise AssertionError("the loader tried to open a socket")

    monkeypatch.setattr(socket, "socket", no_socket)
    monkeypatch.delenv(fid.ENV_WEIGHTS, raising=False)
    with pytest.raises(FileNotFoundError) as e:
        fid.load_inceptionv3_pretrained()
    assert "weights" in str(e.value) and fid.ENV_WEIGHTS in str(e.value)
    monkeypatch.setenv(fid.ENV_WEIGHTS, str(tmp_path / "missing.pth"))
    with pytest.raises(FileNotFoundError, match="missing.pth"):
        fid.load_inceptionv3_pretrained(block_ids=[3])
    # a file named by the environment variable, and a state dict passed directly
    path = tmp_path / "pt_inception.pth"
    torch.save(fixture["sd"], path)
    monkeypatch.setenv(fid.ENV_WEIGHTS, str(path))
    a = fid.load_inceptionv3_pretrained(block_ids=[3])
    b = fid.load_inceptionv3_pretrained(weights=fixture["sd"])
    assert a.output_blocks == [3] and b.output_blocks == [3, 4] and b.last_needed_block == 4
    for k, v in fixture["sd"].items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v)
    bad = dict(fixture["sd"])
    del bad["Mixed_6c.branch7x7_2.conv.weight"]
    with pytest.raises(KeyError, match="Mixed_6c.branch7x7_2.conv.weight"):
        fid.load_inceptionv3_pretrained(weights=bad)


def test_unsupported_arguments_raise():
    from asva_amd import fid
    from asva_amd.evaluation import evaluate_generation_results

    with pytest.raises(NotImplementedError, match="FID variant"):
        fid.InceptionV3((3,), use_fid_inception=False)
    with pytest.raises(NotImplementedError):
        fid.load_inceptionv3_pretrained(use_fid_inception=False, weights={})
    with pytest.raises(ValueError):
        fid.InceptionV3((5,))
    with pytest.raises(ValueError, match="float32"):
        fid.InceptionV3((3,)).to(dtype=torch.float16)
    # eval_fvd=True (the signature's default, as in the reference) is refused before any file is read: the roots do not exist
    with pytest.raises(NotImplementedError, match="eval_fvd=False"):
        evaluate_generation_results("/nonexistent/gt", ["a.mp4"], ["dog"], 1, "/nonexistent/gen", "/nonexistent/out.json", 64)


def test_shim_import_paths_resolve():
    import asva_amd.evaluation as E
    import asva_amd.fid as fid
    from avgen.evaluations.dists import frechet_distance
    from avgen.evaluations.eval import evaluate_generation_results
    from avgen.evaluations.fid import compute_fid_image_features
    from avgen.evaluations.fid.compute_fid import preprocess_images
    from avgen.evaluations.models.inception_v3 import InceptionV3, load_inceptionv3_pretrained

    assert frechet_distance is fid.frechet_distance and evaluate_generation_results is E.evaluate_generation_results
    assert compute_fid_image_features is fid.compute_fid_image_features and preprocess_images is fid.preprocess_images
    assert InceptionV3 is fid.InceptionV3 and load_inceptionv3_pretrained is fid.load_inceptionv3_pretrained


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes

    from asva_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def conv(ldx, ldy, cin=32, cout=32):
        return h.avsd_convnd_ld_f32(p, ldx, p, None, None, None, p, ldy, 1, 1, 4, 4, cin, 1, 4, 4, cout, 1, 1, 1, 1, 1, 1, 0, 0, 0, cin, 0, None)

    assert conv(31, 32) == -1 and b"ldx" in h.avsd_last_error()
    assert conv(32, 31) == -1 and b"ldy" in h.avsd_last_error()
    assert h.avsd_convnd_ld_f32(None, 32, p, None, None, None, p, 32, 1, 1, 4, 4, 32, 1, 4, 4, 32, 1, 1, 1, 1, 1, 1, 0, 0, 0, 32, 0, None) == -1

    def pool(hi, wi, ho, wo, stride, pad, c=8, ldx=8, ldy=8):
        return h.avsd_pool3_hw_f32(p, ldx, p, ldy, 1, hi, wi, c, ho, wo, stride, pad, 0, None)

    assert pool(5, 5, 3, 3, 2, 0) == -1 and b"does not follow" in h.avsd_last_error()        # (5 - 3) / 2 + 1 = 2
    assert pool(5, 5, 4, 5, 1, 1) == -1 and b"does not follow" in h.avsd_last_error()
    assert pool(2, 2, 1, 1, 2, 0) == -1 and b"does not fit" in h.avsd_last_error()
    assert pool(5, 5, 5, 5, 1, 0) == -1 and b"(stride, padding)" in h.avsd_last_error()
    assert pool(5, 5, 5, 5, 1, 1, c=6) == -1 and b"multiple of 4" in h.avsd_last_error()
    assert pool(5, 5, 5, 5, 1, 1, ldx=4) == -1 and b"ldx" in h.avsd_last_error()
    assert pool(5, 5, 5, 5, 1, 1, ldy=10) == -1 and b"ldy" in h.avsd_last_error()
