"""The denoising-loss trainer without a device: the avgen shim, add_noise / get_velocity of every scheduler on CPU tensors against
the float64 formula, argument refusal of the two entry points, the constructor's null-text file, the prob_mask_like rule and the
packing of loss_profile."""
import pytest
import torch

from tests import trainer_ref as R


def _schedulers():
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler

    return [DDIMScheduler, PNDMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler]


def test_shim_exports_the_trainer():
    from avgen.models.trainers import AudioCondAnimationTrainer
    from asva_amd.trainer import AudioCondAnimationTrainer as Native

    assert AudioCondAnimationTrainer is Native


@pytest.mark.parametrize("cls", _schedulers(), ids=lambda c: c.__name__)
def test_add_noise_and_get_velocity_on_cpu_tensors(cls):
    s = cls()
    gen = torch.Generator().manual_seed(3)
    ts = torch.tensor([0, 1, 500, 999])
    tab_a, tab_s = R.tables(s.acp)
    got_a, got_s = s.noise_tables("cpu")
    assert got_a.dtype == got_s.dtype == torch.float32 and got_a.shape == got_s.shape == (1000,)
    assert torch.equal(got_a.double(), tab_a) and torch.equal(got_s.double(), tab_s)
    assert s.noise_tables("cpu")[0] is got_a                                           # cached per device
    # a^2 + s^2 = 1 to f32 rounding: each entry carries a relative error of at most 2^-24, so the sum is off by at most
    # 2 * 2^-24 * (a^2 + s^2) plus second-order terms
    ident = (got_a.double() ** 2 + got_s.double() ** 2 - 1).abs().max().item()
    print(f"MEASURED {cls.__name__}: max |a^2 + s^2 - 1| = {ident:.3e}")
    assert ident <= 2 * 2.0 ** -24 * (1 + 2.0 ** -20)
    for shape in [(4, 4, 3, 5, 6), (4, 7), (4, 3, 2, 2)]:
        x0, noise = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        a, sg = R.coefficients(tab_a, tab_s, ts, ndim=len(shape))
        noisy = s.add_noise(x0, noise, ts)
        vel = s.get_velocity(x0, noise, ts)
        assert noisy.dtype == vel.dtype == torch.float32 and noisy.shape == vel.shape == x0.shape
        assert bool(((noisy.double() - R.add_noise(x0, noise, a, sg)).abs() <= R.elementwise_bound(x0, noise, a, sg)).all())
        assert bool(((vel.double() - R.get_velocity(x0, noise, a, sg)).abs() <= R.elementwise_bound(x0, noise, a, sg, velocity=True)).all())
    x0 = torch.randn(2, 4, generator=gen)
    for bad in ([0, 1000], [-1, 5]):
        with pytest.raises(ValueError, match="range"):
            s.add_noise(x0, x0.clone(), torch.tensor(bad))
        with pytest.raises(ValueError, match="range"):
            s.get_velocity(x0, x0.clone(), torch.tensor(bad))


def test_entry_points_refuse_bad_arguments_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    p = [4096 * (k + 1) * 64 for k in range(8)]          # never dereferenced: every call below is refused before any launch
    x0, noise, ts, ta, tb, noisy, target = p[:7]
    shape = (2, 4, 4, 64)

    def diffuse(x0=x0, noise=noise, ts=ts, ta=ta, tb=tb, T=1000, noisy=noisy, target=target, keep=1, mode=0, shape=shape):
        return h.avsd_diffuse_clip_f32(x0, noise, ts, ta, tb, T, noisy, target, keep, mode, *shape, None)

    for kw in (dict(x0=None), dict(noise=None), dict(ts=None), dict(ta=None), dict(tb=None), dict(noisy=None)):
        assert diffuse(**kw) == -1 and b"null" in h.avsd_last_error()
    for k in range(4):
        bad = tuple(0 if j == k else v for j, v in enumerate(shape))
        assert diffuse(shape=bad) == -1 and b"positive" in h.avsd_last_error()
    assert diffuse(T=0) == -1 and b"T > 0" in h.avsd_last_error()
    assert diffuse(mode=2) == -1 and b"mode" in h.avsd_last_error()
    assert diffuse(noisy=x0) == -1 and b"noisy == x0 is not allowed" in h.avsd_last_error()
    assert diffuse(noisy=x0 + 64) == -1 and b"overlaps" in h.avsd_last_error()
    assert diffuse(target=noise) == -1 and b"target overlaps" in h.avsd_last_error()
    assert diffuse(target=noisy + 4) == -1 and b"noisy and target overlap" in h.avsd_last_error()
    assert diffuse(noisy=noisy + 2) == -1 and b"aligned" in h.avsd_last_error()

    pred, tgt, scratch, per, loss = p[:5]

    def mse(pred=pred, tgt=tgt, f0=1, scratch=scratch, per=per, loss=loss, shape=shape):
        return h.avsd_frame_mse_f32(pred, tgt, f0, scratch, per, loss, *shape, None)

    for kw in (dict(pred=None), dict(tgt=None), dict(scratch=None), dict(per=None), dict(loss=None)):
        assert mse(**kw) == -1 and b"null" in h.avsd_last_error()
    for k in range(4):
        bad = tuple(0 if j == k else v for j, v in enumerate(shape))
        assert mse(shape=bad) == -1 and b"positive" in h.avsd_last_error()
    assert mse(f0=4) == -1 and b"no frames to score" in h.avsd_last_error()               # F - f0 == 0
    assert mse(f0=1, shape=(2, 4, 1, 64)) == -1 and b"no frames to score" in h.avsd_last_error()
    assert mse(f0=-1) == -1 and b"no frames to score" in h.avsd_last_error()
    assert mse(per=pred + 16) == -1 and b"overlaps an input" in h.avsd_last_error()
    assert mse(loss=scratch + 8) == -1 and b"overlap" in h.avsd_last_error()


def test_ops_wrappers_refuse_before_any_launch():
    from asva_amd import ops

    x = torch.zeros(1, 4, 2, 2, 2)
    with pytest.raises(ValueError, match="device tensor"):
        ops.frame_mse(x, x.clone())
    with pytest.raises(ValueError, match="range"):
        ops.check_timesteps(torch.tensor([3, 1000]), 2, 1000, "cpu")
    with pytest.raises(ValueError, match="vector of 2"):
        ops.check_timesteps(torch.tensor([3]), 2, 1000, "cpu")
    assert ops.check_timesteps(torch.tensor([3, 999]), 2, 1000, "cpu").dtype == torch.int32


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    device = property(lambda self: self.w.device)
    dtype = property(lambda self: self.w.dtype)


def _stub_trainer(**kw):
    from asva_amd.schedulers import PNDMScheduler
    from asva_amd.trainer import AudioCondAnimationTrainer

    kw.setdefault("null_text_encoding", torch.zeros(7, 64))
    return AudioCondAnimationTrainer(_Stub(), _Stub(), _Stub(), PNDMScheduler(), **kw)


def test_constructor_null_text_encoding(tmp_path):
    from asva_amd.schedulers import PNDMScheduler
    from asva_amd.trainer import NULL_TEXT_ENCODING_PATH, AudioCondAnimationTrainer

    assert NULL_TEXT_ENCODING_PATH == "pretrained/openai-clip-l_null_text_encoding.pt"
    missing = tmp_path / "absent" / "null.pt"
    with pytest.raises(FileNotFoundError, match="null.pt") as e:
        _stub_trainer(null_text_encoding=str(missing))
    assert str(missing) in str(e.value)
    enc = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(0))
    torch.save(enc, tmp_path / "null.pt")
    t = AudioCondAnimationTrainer(_Stub(), _Stub(), _Stub(), PNDMScheduler(), null_text_encoding=tmp_path / "null.pt")
    assert t.null_text_encoding.shape == (1, 1, 77, 768) and not t.null_text_encoding.requires_grad
    assert torch.equal(t.null_text_encoding[0, 0], enc[0])
    assert t.device == torch.device("cpu") and t.dtype == torch.float32
    assert (t.text_cond_drop_prob, t.audio_cond_drop_prob, t.loss_on_first_frame) == (0.0, 0.0, False)


def test_prob_mask_like_rule():
    from asva_amd.trainer import keep_masks, prob_mask_like

    assert bool(prob_mask_like((5,), 1, "cpu").all()) and prob_mask_like((5,), 1.0, "cpu").dtype == torch.bool
    assert not bool(prob_mask_like((5,), 0, "cpu").any())
    g1, g2 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    m = prob_mask_like((4096,), 0.25, "cpu", g1)
    assert torch.equal(m, R.prob_mask_like((4096,), 0.25, g2))                         # uniform(0, 1) < prob
    assert 0.2 < m.float().mean().item() < 0.3
    # training: keep probability = 1 - drop probability; eval: everything is kept whatever the probabilities are
    t, a = keep_masks(6, True, 1.0, 0.0, "cpu")
    assert not bool(t.any()) and bool(a.all())
    t, a = keep_masks(6, True, 0.0, 1.0, "cpu")
    assert bool(t.all()) and not bool(a.any())
    for probs in [(1.0, 1.0), (0.5, 0.5), (0.0, 0.0)]:
        t, a = keep_masks(6, False, *probs, "cpu")
        assert bool(t.all()) and bool(a.all())


@pytest.mark.parametrize("rows", [1, 4, 8])
def test_loss_profile_packing_is_a_partition(rows):
    from asva_amd.trainer import pack_rows

    chunks = pack_rows(5, 3, rows)
    assert all(1 <= len(c) <= rows for c in chunks)
    flat = [p for c in chunks for p in c]
    assert sorted(flat) == [(t, b) for t in range(5) for b in range(3)] and len(set(flat)) == 15
    assert chunks == pack_rows(5, 3, rows)                                              # a pure function
    assert len(chunks) == -(-15 // rows)
    with pytest.raises(ValueError):
        pack_rows(5, 3, 0)


def test_unknown_prediction_type_raises_as_in_the_reference():
    t = _stub_trainer()
    t.scheduler.config["prediction_type"] = "sample"
    with pytest.raises(ValueError, match="Unknown prediction type sample"):
        t._mode()
    t.scheduler.config["prediction_type"] = "v_prediction"
    assert t._mode() == "v_prediction"


def test_unrotated_k_walk_restores_the_setting():
    from asva_amd import ops
    from asva_amd.trainer import unrotated_k_walk

    before = ops._KROT
    try:
        for start in (True, False):
            ops.set_krot(start)
            with unrotated_k_walk():
                assert ops._KROT is False
            assert ops._KROT is start
            with pytest.raises(RuntimeError):
                with unrotated_k_walk():
                    raise RuntimeError("a forward failed")
            assert ops._KROT is start
    finally:
        ops.set_krot(before)
