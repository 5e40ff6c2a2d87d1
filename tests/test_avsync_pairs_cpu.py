"""The AVSync classifier on a matrix of pairs without a GPU (-m "not gpu"): clip timing in closed form, `pair_scores` through the
torch backend against the materialised float64 restatement (tests/avsync_pairs_ref.py), the contrastive trainer's axes, labels and
tau, and the evaluation's reduction rule.

Bounds: the torch backend is fp32 CPU arithmetic on a three-layer head, the restatement float64 -> scores within 1e-5 (1 + |s|), the
bound tests/test_avsync_gpu.py derives for the whole classifier; losses move at most twice the logit error over tau.
"""
import random

import numpy as np
import pytest
import torch

from tests import avsync_pairs_ref as PR
from tests import avsync_ref as R
from tests.helpers import load_golden, load_shapes


def _net(dim=512, sd_head=None):
    from asva_amd import avsync as A

    net = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead(dim=dim)).eval()
    if sd_head is not None:
        net.head.load_state_dict(sd_head)
    return net


# ---- clip timing -------------------------------------------------------------------------------------------------------------------------
def test_center_compact_starts_in_closed_form():
    from asva_amd import avsync as A

    # a 10 s recording, 2 s clips: starts range over [0, 8]; 31 clips 0.04 s apart span 1.2 s, centred: (8 - 1.2) / 2 = 3.4
    s = A.clip_starts(0.0, 10.0 - 2.0, 31, 0.04, "center-compact")
    assert s.dtype == np.float64 and s.shape == (31,)
    assert abs(s[0] - 3.4) < 1e-12 and abs(s[-1] - 4.6) < 1e-12 and np.allclose(np.diff(s), 0.04, atol=1e-12)
    assert abs(s[15] - 4.0) < 1e-12                                  # the centre clip sits in the middle of the range
    t = A.clip_frame_seconds(s, 12, 6)
    assert t.shape == (31, 13)
    assert abs(t[0, 0] - 3.4001) < 1e-12 and abs(t[0, 1] - (3.4 + 1 / 6)) < 1e-12 and abs(t[0, -1] - 5.3999) < 1e-12


def test_uniform_with_and_without_endpoint():
    from asva_amd import avsync as A

    assert np.allclose(A.uniform_starts(0.0, 8.0, 5, endpoint=True), [0, 2, 4, 6, 8], atol=1e-12)
    assert np.allclose(A.uniform_starts(0.0, 8.0, 4, endpoint=False), [1, 3, 5, 7], atol=1e-12)
    assert np.allclose(A.clip_starts(0.0, 8.0, 5, 0.04, "uniform"), [0, 2, 4, 6, 8], atol=1e-12)
    # uniform does not look at the gap: a range too short for the compact types still spreads
    assert np.allclose(A.clip_starts(0.0, 1.0, 3, 10.0, "uniform"), [0, 0.5, 1.0], atol=1e-12)


def test_too_short_a_range_is_refused():
    from asva_amd import avsync as A

    for kind in ("center-compact", "random-compact", "random"):
        with pytest.raises(ValueError, match="cannot hold"):
            A.clip_starts(0.0, 1.0, 31, 0.04, kind)                   # 30 x 0.04 = 1.2 > 1
        assert A.clip_starts(0.0, 1.2, 31, 0.04, kind, rng=random.Random(0)).shape == (31,)        # exactly enough
    with pytest.raises(ValueError, match="sampling"):
        A.clip_starts(0.0, 8.0, 3, 0.04, "centre")


def test_random_types_keep_their_promises():
    from asva_amd import avsync as A

    rng = random.Random(3)
    s = A.clip_starts(1.0, 9.0, 7, 0.2, "random-compact", rng=rng)
    assert np.allclose(np.diff(s), 0.2, atol=1e-12) and s[0] >= 1.0 and s[-1] <= 9.0
    s = A.clip_starts(1.0, 9.0, 7, 0.2, "random", rng=rng)
    assert (np.diff(s) >= 0.2 - 1e-12).all() and s[0] >= 1.0 and s[-1] <= 9.0
    again = A.clip_starts(1.0, 9.0, 7, 0.2, "random", rng=random.Random(3))
    assert A.clip_starts(1.0, 9.0, 7, 0.2, "random", rng=random.Random(3)).tolist() == again.tolist()


@pytest.mark.parametrize("fps", [25, 30])
def test_nearest_frame_pick(fps):
    from asva_amd import avsync as A

    stamps = np.arange(10 * fps, dtype=np.float64) / fps
    want = lambda t: int(np.floor(t * fps + 0.5))  # noqa: E731
    times = np.array([3.4001, 3.4 + 1 / 6, 3.4 + 2 / 6, 5.2333, 0.0, 9.93])
    got = A.nearest_frames(times, stamps)
    assert got.tolist() == [min(want(t), 10 * fps - 1) for t in times]
    # exactly between two frames (representable: stamps k / fps and (k + 1) / fps with a dyadic midpoint): the earlier frame
    st = np.array([0.0, 0.25, 0.5, 0.75])
    assert A.nearest_frames(np.array([0.125, 0.375, 0.625]), st).tolist() == [0, 1, 2]
    assert A.nearest_frames(np.array([[0.126], [0.374]]), st).tolist() == [[1], [1]]


# ---- pair_scores through the torch backend ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 3), (3, 5, 7)])
@pytest.mark.parametrize("dim", [512, 64, 48])            # the fused route twice, and a head size that takes the materialised route
def test_pair_scores_against_materialised_restatement(shape, dim):
    G, P, Q = shape
    sd = PR.draw_head(dim, 11 + dim)
    net = _net(dim, sd)
    a, v = PR.draw_embeddings(G, P, Q, dim, 5)
    want = PR.pair_scores64(sd, a, v)
    got = net.pair_scores(a, v, be=PR.TorchBackend)
    assert got.shape == (G, P, Q) and got.dtype == torch.float32
    bound = 1e-5 * (1.0 + want.abs())
    assert bool(((got.double() - want).abs() <= bound).all()), (got.double() - want).abs().max()
    # the test can tell a wrong layout: audio and video swapped, or the pair matrix transposed, lies far outside the bound
    if P == Q:
        assert not bool(((got.double().transpose(1, 2) - want).abs() <= bound).all())
        swapped = net.pair_scores(v, a, be=PR.TorchBackend)
        assert not bool(((swapped.double() - want).abs() <= bound).all())
        assert not bool(((swapped.double().transpose(1, 2) - want).abs() <= bound).all())       # W1's halves are not interchangeable
    else:
        assert net.pair_scores(v, a, be=PR.TorchBackend).shape == (G, Q, P)
    # the aligned rows are what score_embeddings' route gives
    from asva_amd import avsync as A

    k = min(P, Q)
    diag = A.run_head(A.fold_head(net.head), a[:, :k].reshape(G * k, dim), v[:, :k].reshape(G * k, dim), PR.TorchBackend)[:, 0].reshape(G, k)
    assert bool(((diag.double() - want[:, :k, :k].diagonal(dim1=1, dim2=2)).abs() <= 1e-5 * (1.0 + diag.abs())).all())


def test_pair_scores_refuses_bad_shapes():
    net = _net(64, PR.draw_head(64, 1))
    with pytest.raises(ValueError, match="pair_scores"):
        net.pair_scores(torch.zeros(2, 3, 64), torch.zeros(3, 3, 64), be=PR.TorchBackend)
    with pytest.raises(ValueError, match="pair_scores"):
        net.pair_scores(torch.zeros(2, 3, 64), torch.zeros(2, 3, 32), be=PR.TorchBackend)
    with pytest.raises(ValueError, match="pair_scores"):
        net.pair_scores(torch.zeros(6, 64), torch.zeros(6, 64), be=PR.TorchBackend)
    with pytest.raises(ValueError, match="empty"):
        net.pair_scores(torch.zeros(2, 0, 64), torch.zeros(2, 3, 64), be=PR.TorchBackend)


def test_route_follows_the_head_size():
    from asva_amd import ops

    assert ops.pair_head_supported(512, 512, 256) and ops.pair_head_supported(64, 64, 32) and ops.pair_head_supported(32, 96, 96)
    assert not ops.pair_head_supported(48, 48, 24) and not ops.pair_head_supported(1024, 1024, 512) and not ops.pair_head_supported(64, 64, 48)


# ---- the contrastive trainer ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    g = load_golden("avsync_tiny.pt")
    sd = R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    R.check_draw(sd, g["probe"])
    return g, sd


@pytest.mark.parametrize("tau", [1.0, 0.07])
def test_contrastive_trainer_against_restatement(tiny, tau):
    from asva_amd import avsync as A
    from tests.test_avsync_cpu import _TorchBackend

    class Be(_TorchBackend, PR.TorchBackend):          # convolutions of the encoders + the pair entry points
        pass

    g, sd = tiny
    net = _net()
    net.load_state_dict(sd)
    audios, videos = PR.tiny_clips(g["audio"])
    trainer = A.AVSyncContrastiveTrainer(net.audio_encoder, net.video_encoder, net.head, tau=tau)
    got = trainer(audios, videos, be=Be)
    assert all(t.dim() == 0 and t.dtype == torch.float32 and not t.requires_grad for t in got)
    a64, v64 = PR.tiny_reference(sd, audios, videos)
    s64 = PR.pair_scores64(R._sub(sd, "head."), a64, v64)
    want = PR.contrastive64(s64, tau)
    bound = 2e-5 * (1.0 + float(s64.abs().max())) / tau
    assert abs(float(got[0]) - float(want[0])) <= bound and abs(float(got[1]) - float(want[1])) <= bound, (got, want)
    # which axis is av: the objective of the transposed matrix swaps the two losses, and they differ by far more than the bound
    assert abs(float(want[0]) - float(want[1])) > 10 * bound
    assert PR.top2_margin(s64) > 4e-5 * (1.0 + float(s64.abs().max())) and PR.top2_margin(s64.transpose(1, 2)) > 4e-5 * (1.0 + float(s64.abs().max()))
    assert float(got[2]) == float(want[2].float()) and float(got[3]) == float(want[3].float())      # the same count over b k, as an f32


def test_trainer_labels_axes_and_tau_on_given_scores(monkeypatch):
    """AVSyncContrastiveTrainer.forward on a score matrix where the answer is known (the encoders and pair_scores replaced by the given
    matrix): which result is av and which va, the aligned pair as the label, and `tau` reaching the objective"""
    from asva_amd import avsync as A

    b, k = 2, 4
    s = torch.zeros(b, k, k) + 3.0 * torch.eye(k)
    monkeypatch.setattr(A, "_embed_pairs", lambda net, audios, videos, be: (None, None))
    monkeypatch.setattr(A.AVSyncClassifier, "pair_scores", lambda self, a, v, be=None: s)
    trainer = A.AVSyncContrastiveTrainer(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead(dim=64), tau=1.0)
    got = trainer(None, None, be=PR.TorchBackend)
    assert float(got[2]) == 1.0 and float(got[3]) == 1.0                     # a strong diagonal: every audio picks its video and back
    # audio 0 of example 0 prefers video 1; audios 2 and 3 of example 1 prefer video 0, whose own best audio becomes 3:
    # av loses 3 of 8 rows, va loses column 1 of example 0 and column 0 of example 1
    s[0, 0, 1], s[1, 2, 0], s[1, 3, 0] = 5.0, 4.0, 4.5
    for tau in (1.0, 0.5, 0.07):
        trainer.tau = tau
        got, want = trainer(None, None, be=PR.TorchBackend), PR.contrastive64(s, tau)
        assert float(got[2]) == 5 / 8 == float(want[2]) and float(got[3]) == 6 / 8 == float(want[3])
        for i in (0, 1):
            assert abs(float(got[i]) - float(want[i])) < 1e-5 * (1 + float(want[i])), (tau, i)
        assert abs(float(want[0]) - float(want[1])) > 1e-2                   # av and va losses are told apart
    assert float(PR.contrastive64(s, 0.07)[0]) > 2 * float(PR.contrastive64(s, 1.0)[0])          # tau divides the logits


def test_trainer_save_pretrained_and_import_path(tmp_path):
    from asva_amd import avsync as A
    from avsync.models.sync_contrastive_trainer import AVSyncContrastiveTrainer

    assert AVSyncContrastiveTrainer is A.AVSyncContrastiveTrainer
    t = AVSyncContrastiveTrainer(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead(), tau=0.5)
    assert t.tau == 0.5 and "Values only".lower() in AVSyncContrastiveTrainer.__doc__.lower()
    assert sorted(k.split(".")[0] for k in t.state_dict()) and {k.split(".")[0] for k in t.state_dict()} == {"audio_encoder", "video_encoder", "head"}
    t.save_pretrained(str(tmp_path))
    for sub in ("audio_encoder", "video_encoder", "head"):
        assert (tmp_path / sub / "config.json").is_file()
    again = A.load_avsync_model(str(tmp_path))
    assert all(torch.equal(v, again.head.state_dict()[k]) for k, v in t.head.state_dict().items())


# ---- the evaluation ---------------------------------------------------------------------------------------------------------------------------
class _FakeNet:
    """a classifier whose predictions are given: evaluate_shift_accuracy only reduces"""


def _patched_eval(monkeypatch, preds):
    """evaluate_shift_accuracy with shift_accuracy replaced by a table {batch audio tag: (av_pred, va_pred)}"""
    from asva_amd import avsync as A

    def fake(net, audios, videos, tolerate_range=5, be=None):
        av, va = preds[int(audios[0, 0, 0, 0, 0])]
        c = audios.shape[1] // 2
        av, va = torch.tensor(av), torch.tensor(va)
        return {"av_pred": av, "va_pred": va, "av_hit": (av - c).abs() <= tolerate_range, "va_hit": (va - c).abs() <= tolerate_range}

    monkeypatch.setattr(A, "shift_accuracy", fake)
    return A.evaluate_shift_accuracy


def _batch(tag, indices, k):
    return {"index": torch.tensor(indices), "audio": torch.full((len(indices), k, 1, 1, 1), float(tag)), "video": torch.zeros(len(indices), k, 3, 1, 1, 1)}


def test_duplicates_count_once_and_the_first_occurrence_wins(monkeypatch):
    k, c = 31, 15
    # example 4 appears in batch 0 as a hit (both ways) and in batch 1 as a miss: the hit counts
    preds = {0: ([c, c + 9, c], [c, c, c - 9]), 1: ([c + 9, c], [c + 9, c])}
    ev = _patched_eval(monkeypatch, preds)
    r = ev(_FakeNet(), [_batch(0, [4, 7, 2], k), _batch(1, [4, 9], k)], tolerate_range=5)
    want = PR.reduce_unique([4, 7, 2, 4, 9], [1, 0, 1, 0, 1], [1, 1, 0, 0, 1])
    assert r["valid_examples"] == 4 == want[2]
    assert r["av_acc"] == want[0] == 3 / 4 and r["va_acc"] == want[1] == 3 / 4


def test_tolerance_is_inclusive_and_even_k_uses_k_over_2(monkeypatch):
    k = 8                                               # centre index 4
    preds = {0: ([4 + 2, 4 - 2, 4 + 3, 4 - 3], [4 - 2, 4 + 2, 4 - 3, 4 + 3])}
    ev = _patched_eval(monkeypatch, preds)
    r = ev(_FakeNet(), [_batch(0, [0, 1, 2, 3], k)], tolerate_range=2)
    assert r["av_acc"] == 0.5 and r["va_acc"] == 0.5 and r["valid_examples"] == 4      # |d| == 2 hits, |d| == 3 misses


def test_shift_accuracy_against_restatement_on_embeddings(monkeypatch):
    """shift_accuracy's own logic (centre k // 2, P = 1 and Q = 1 calls, which argmax is av) with the encoders replaced by given embeddings"""
    from asva_amd import avsync as A

    for k in (5, 4):
        b, dim = 3, 64
        sd = PR.draw_head(dim, 23)
        net = _net(dim, sd)
        a, v = PR.draw_embeddings(b, k, k, dim, 40 + k)
        calls = []
        monkeypatch.setattr(A, "_embed_pairs", lambda net, audios, videos, be: (a, v))
        real = A.AVSyncClassifier.pair_scores

        def spy(self, x, y, be=None):
            calls.append((tuple(x.shape), tuple(y.shape)))
            return real(self, x, y, be)

        monkeypatch.setattr(A.AVSyncClassifier, "pair_scores", spy)
        want = PR.shift_eval64(sd, a, v, 1)
        assert PR.top2_margin(want["av_scores"]) > 4e-5 * (1 + float(want["av_scores"].abs().max()))
        assert PR.top2_margin(want["va_scores"]) > 4e-5 * (1 + float(want["va_scores"].abs().max()))
        got = A.shift_accuracy(net, None, None, tolerate_range=1, be=PR.TorchBackend)
        assert calls == [((b, 1, dim), (b, k, dim)), ((b, k, dim), (b, 1, dim))]
        for key in ("av_pred", "va_pred", "av_hit", "va_hit"):
            assert got[key].tolist() == want[key].tolist(), key
        assert not torch.equal(want["av_pred"], want["va_pred"])          # the case can tell av from va
        monkeypatch.undo()


def test_measured_figures_lie_inside_the_bounds():
    """tests/golden/avsync_pairs_measured.json: what tests/test_avsync_pairs_gpu.py measured on the MI355X, against the bounds it asserts"""
    import json
    import os

    from tests.helpers import GOLDEN

    with open(os.path.join(GOLDEN, "avsync_pairs_measured.json")) as f:
        m = json.load(f)["gpu"]
    assert 0 < m["pair_scores_vs_float64_rel"] <= 1e-5 and 0 < m["pair_scores_vs_score_embeddings_rel"] <= 2e-5
    assert 0 < m["pair_xent_loss_rel"] <= 1e-5
    assert all(0 < v <= 1e-5 for k, v in m.items() if k.startswith("pair_scores_dim"))
