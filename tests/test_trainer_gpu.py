"""The denoising loss on the MI355X (-m gpu): avsd_diffuse_clip_f32 and avsd_frame_mse_f32 inside NaN-poisoned memory against
tests/trainer_ref.py, AudioCondAnimationTrainer on the tiny UNet / VAE against the same restatement and against the fp32 CPU
oracle of the UNet, loss_profile's independence of its packing, and the schedulers' add_noise on device tensors.

Bounds.  Noising: 3 * 2^-24 * (|a x0| + |s n|) per element (one rounding per product, one for the sum, contracted or not).
Reduction: any f32 summation order of n non-negative terms, each the square of one rounded difference, is within
(n + 2) u / (1 - (n + 2) u) of float64, u = 2^-24 (tests/trainer_ref.py mse_bound); the measured error is printed.  On an MI355X
the relative error of per_sample at f0 = 0 / f0 = 1 was 2.6e-9 / 3.0e-8 for (1, 4, 2, 1, 1), 8.8e-9 / 5.1e-9 for (2, 3, 3, 5, 7),
5.4e-8 / 5.3e-8 for (3, 4, 4, 8, 8) and 1.7e-8 / 2.4e-8 for (2, 4, 12, 32, 32).
UNet: tests/test_unet_gpu.py holds every sample of the tiny network to rel-L2 3e-2 (bf16) / 5e-3 (fp16 + f32 residual) of the
fp32 reference, so by the triangle inequality |sqrt(per_sample[b]) - rms_ref[b]| <= tol * ||pred_ref[b]|| / sqrt(n)."""
import warnings

import pytest
import torch

from tests import trainer_ref as R
from tests.helpers import filled_unet, load_golden
from tests.test_host_cpu import TINY_VAE, _filled_vae

pytestmark = pytest.mark.gpu


def _poisoned(src, pad):
    """`src` copied into the middle of a NaN-filled allocation, `pad` floats in: rows are 4-byte aligned only"""
    n = src.numel()
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    view = buf[pad:pad + n].view(src.shape)
    view.copy_(src)
    return view, buf


def _nan_out(shape, pad):
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    return buf[pad:pad + n].view(shape), buf


def _untouched(buf, pad):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[buf.numel() - pad:]).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _both_libraries(fn):
    """fn() under the bf16 and the fp16 library -> [result, result]"""
    from asva_amd import precision

    out = []
    try:
        for name in ("bf16", "fp16"):
            precision.set_precision(name)
            out.append(fn())
    finally:
        precision.set_precision("bf16")
    return out


@pytest.fixture(scope="module")
def tables():
    from asva_amd.schedulers import PNDMScheduler

    return PNDMScheduler().noise_tables("cuda")


# ---- avsd_diffuse_clip_f32 -------------------------------------------------------------------------------------------------
DIFFUSE_SHAPES = [(1, 4, 2, 1, 1), (2, 4, 4, 3, 5), (1, 3, 1, 2, 3), (3, 4, 4, 8, 8), (1, 4, 12, 8, 8)]


def _timesteps(shape):
    return [0, 500, 999] if shape[0] == 3 else [(731 * (b + 1) + shape[2]) % 1000 for b in range(shape[0])]


@pytest.mark.parametrize("shape", DIFFUSE_SHAPES)
@pytest.mark.parametrize("keep_first", [False, True])
@pytest.mark.parametrize("mode", ["epsilon", "v"])
def test_diffuse_clip_in_poisoned_memory(shape, keep_first, mode, tables):
    from asva_amd import ops

    gen = torch.Generator().manual_seed(shape[0] * 1000 + shape[2] * 10 + shape[3])
    x0_h, noise_h = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    ts = torch.tensor(_timesteps(shape))
    x0, xbuf = _poisoned(x0_h, 37)
    noise, nbuf = _poisoned(noise_h, 5)
    a, s = R.coefficients(tables[0], tables[1], ts)
    want_noisy, want_target = R.noisy_and_target(x0_h, noise_h, a, s, keep_first, "epsilon" if mode == "epsilon" else "v_prediction")

    def run():
        noisy, obuf = _nan_out(shape, 3)
        target, tbuf = _nan_out(shape, 9)
        got = ops.diffuse_clip(x0, noise, ts, tables[0], tables[1], keep_first=keep_first, mode=mode, noisy=noisy, target=target)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == noisy.data_ptr() and got[1].data_ptr() == target.data_ptr()
        assert _untouched(obuf, 3) and _untouched(tbuf, 9)                               # the padding is still NaN
        return noisy.clone(), target.clone()

    (noisy, target), (noisy16, target16) = _both_libraries(run)
    assert torch.equal(_bits(noisy), _bits(noisy16)) and torch.equal(_bits(target), _bits(target16))      # both libraries, same bits
    assert torch.equal(_bits(x0), _bits(x0_h.cuda())) and torch.equal(_bits(noise), _bits(noise_h.cuda()))  # inputs are read only
    assert _untouched(xbuf, 37) and _untouched(nbuf, 5)
    if keep_first:
        assert torch.equal(_bits(noisy[:, :, 0]), _bits(x0[:, :, 0]))                    # frame 0 is the clean latent, in bits
    f0 = 1 if keep_first else 0
    err = (noisy.double().cpu() - want_noisy).abs()[:, :, f0:]
    assert bool((err <= R.elementwise_bound(x0_h, noise_h, a, s)[:, :, f0:]).all())
    if mode == "epsilon":
        assert torch.equal(_bits(target), _bits(noise))                                  # every frame, frame 0 included
    else:
        err = (target.double().cpu() - want_target).abs()
        assert bool((err <= R.elementwise_bound(x0_h, noise_h, a, s, velocity=True)).all())
    # a null target: the caller uses noise itself
    only, none = ops.diffuse_clip(x0, noise, ts, tables[0], tables[1], keep_first=keep_first, mode=mode, want_target=False)
    assert none is None and torch.equal(_bits(only), _bits(noisy))


def test_diffuse_clip_validates_timesteps_and_overlaps(tables):
    from asva_amd import _lib, ops

    shape = (2, 4, 2, 4, 4)
    x0, noise = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
    for bad in (torch.tensor([5, 1000]), torch.tensor([-1, 5], device="cuda"), torch.tensor([5]), torch.tensor([0.5, 1.0])):
        with pytest.raises(ValueError, match="timesteps"):
            ops.diffuse_clip(x0, noise, bad, *tables)
    with pytest.raises(ValueError, match="overlaps an input"):
        ops.diffuse_clip(x0, noise, torch.tensor([5, 6]), *tables, noisy=x0)
    with pytest.raises(ValueError, match="mode"):
        ops.diffuse_clip(x0, noise, torch.tensor([5, 6]), *tables, mode="sample")
    # the kernel itself writes nothing for a sample whose timestep is out of range (and never indexes the tables with it)
    noisy, obuf = _nan_out(shape, 3)
    ts = torch.tensor([5, 1000], dtype=torch.int32, device="cuda")
    rc = _lib.lib().avsd_diffuse_clip_f32(x0.data_ptr(), noise.data_ptr(), ts.data_ptr(), tables[0].data_ptr(), tables[1].data_ptr(), 1000,
                                          noisy.data_ptr(), None, 1, 0, 2, 4, 2, 16, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(noisy[1]).all()) and not bool(torch.isnan(noisy[0]).any()) and _untouched(obuf, 3)


# ---- avsd_frame_mse_f32 ----------------------------------------------------------------------------------------------------
MSE_SHAPES = [(1, 4, 2, 1, 1), (2, 3, 3, 5, 7), (3, 4, 4, 8, 8), (2, 4, 12, 32, 32)]


@pytest.mark.parametrize("shape", MSE_SHAPES)
@pytest.mark.parametrize("f0", [0, 1])
def test_frame_mse_in_poisoned_memory(shape, f0):
    from asva_amd import ops

    B, C, F, H, W = shape
    gen = torch.Generator().manual_seed(B * 1000 + F * 10 + H + f0)
    pred_h, target_h = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    pred, pbuf = _poisoned(pred_h, 37)
    target, tbuf = _poisoned(target_h, 5)
    want_loss, want_per = R.sliced_mse(pred_h, target_h, loss_on_first_frame=f0 == 0)
    n = C * (F - f0) * H * W

    def run():
        loss, per = ops.frame_mse(pred, target, f0)
        torch.cuda.synchronize()
        return loss.clone(), per.clone()

    (loss, per), (loss16, per16) = _both_libraries(run)
    assert loss.shape == () and per.shape == (B,) and loss.dtype == per.dtype == torch.float32 and loss.is_cuda
    assert torch.equal(_bits(loss), _bits(loss16)) and torch.equal(_bits(per), _bits(per16))        # both libraries, same bits
    loss2, per2 = run()
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(per), _bits(per2))          # two calls, same bits
    assert torch.equal(_bits(pred), _bits(pred_h.cuda())) and torch.equal(_bits(target), _bits(target_h.cuda()))
    assert _untouched(pbuf, 37) and _untouched(tbuf, 5)
    rel_per = ((per.double().cpu() - want_per).abs() / want_per).max().item()
    rel_loss = abs(loss.double().item() - want_loss.item()) / want_loss.item()
    print(f"MEASURED frame_mse {shape} f0={f0}: n = {n}, per_sample rel err {rel_per:.3e}, loss rel err {rel_loss:.3e}, "
          f"bound {R.mse_bound(n):.3e}")
    assert rel_per <= R.mse_bound(n) and rel_loss <= R.mse_bound(n)
    # per_sample[b] depends neither on B nor on the sample's position in the batch
    for b in range(B):
        alone = ops.frame_mse(pred[b:b + 1], target[b:b + 1], f0)[1]
        assert torch.equal(_bits(alone), _bits(per[b:b + 1]))
    zero_loss, zero_per = ops.frame_mse(pred, pred.clone(), f0)
    assert zero_loss.item() == 0.0 and bool((zero_per == 0).all())


def test_frame_mse_refuses_an_empty_slice():
    from asva_amd import ops

    x = torch.zeros(1, 4, 1, 2, 2, device="cuda")
    with pytest.raises(ValueError, match="no frames to score"):
        ops.frame_mse(x, x.clone(), 1)
    assert ops.frame_mse(x, x.clone(), 0)[0].item() == 0.0


# ---- the trainer on the tiny network ---------------------------------------------------------------------------------------
class _TinyAudioEncoder(torch.nn.Module):
    """stand-in for ImageBindSegmaskAudioEncoder: audios (b, 229, 8) -> encodings (b, 229, 64) and audio_segment_mask(4); the bias makes
    the encodings of silence (the null branch) differ from zero and from the real ones"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.w = torch.nn.Parameter(torch.randn(8, 64, generator=g) * 0.4, requires_grad=False)
        self.b = torch.nn.Parameter(torch.randn(64, generator=g) * 0.5, requires_grad=False)

    def forward(self, audios, return_dict=False):
        from asva_amd.conditioning import audio_segment_mask

        enc = torch.tanh(audios.float() @ self.w + self.b)
        masks = audio_segment_mask(4).to(enc.device)[None].expand(enc.shape[0], -1, -1).contiguous()
        return enc.mean(1), enc, masks


TIMESTEPS = [981, 1]


class _Tiny:
    def __init__(self):
        self.g = load_golden("unet_tiny_e2e.pt")
        gen = torch.Generator().manual_seed(5)
        self.videos = torch.rand(2, 3, 4, 64, 64, generator=gen)
        self.audios = torch.randn(2, 229, 8, generator=gen)
        self.text = self.g["text"].clone()                                   # (2, 7, 64)
        self.null_text = torch.randn(7, 64, generator=gen)
        self.sd = None

    def trainer(self, f32_residual=False, **kw):
        from asva_amd.schedulers import PNDMScheduler
        from asva_amd.trainer import AudioCondAnimationTrainer

        unet = filled_unet(self.g["config"])
        if self.sd is None:
            self.sd = {k: v.clone() for k, v in unet.state_dict().items()}
        unet = unet.to("cuda")
        unet.f32_residual = f32_residual
        t = AudioCondAnimationTrainer(_filled_vae(TINY_VAE).to("cuda"), _TinyAudioEncoder().to("cuda"), unet, PNDMScheduler(),
                                      null_text_encoding=self.null_text, **kw)
        return t.eval()

    def forward(self, trainer, **kw):
        kw.setdefault("timesteps", torch.tensor(TIMESTEPS))
        kw.setdefault("generator", torch.Generator().manual_seed(17))
        kw.setdefault("videos", self.videos)
        kw.setdefault("audios", self.audios)
        kw.setdefault("text_encodings", self.text)
        return trainer(kw.pop("videos"), kw.pop("audios"), kw.pop("text_encodings"), return_parts=True, **kw)


@pytest.fixture(scope="module")
def tiny():
    return _Tiny()


def _check_against_restatement(trainer, loss, parts, tables):
    lat, noise, ts = parts["latents"], parts["noise"], parts["timesteps"]
    assert lat.shape == (2, 4, 4, 8, 8) and lat.dtype == torch.float32
    a, s = R.coefficients(tables[0], tables[1], ts)
    want_noisy, want_target = R.noisy_and_target(lat.cpu(), noise.cpu(), a, s, True, "epsilon")
    noisy = parts["noisy_latents"]
    assert torch.equal(_bits(noisy[:, :, 0]), _bits(lat[:, :, 0]))                       # (b) frame 0 is the clean latent, bit for bit
    assert bool(((noisy.double().cpu() - want_noisy).abs() <= R.elementwise_bound(lat.cpu(), noise.cpu(), a, s)).all())
    assert torch.equal(_bits(parts["target"]), _bits(noise))
    want_loss, want_per = R.sliced_mse(parts["prediction"], want_target, trainer.loss_on_first_frame)
    n = 4 * (4 - (0 if trainer.loss_on_first_frame else 1)) * 64
    rel_per = ((parts["per_sample"].double().cpu() - want_per).abs() / want_per).max().item()
    rel_loss = abs(loss.double().item() - want_loss.item()) / want_loss.item()
    print(f"MEASURED trainer loss_on_first_frame={trainer.loss_on_first_frame}: loss {loss.item():.6f}, per_sample "
          f"{parts['per_sample'].tolist()}, rel err {rel_per:.3e} / {rel_loss:.3e}, bound {R.mse_bound(n):.3e}")
    assert rel_per <= R.mse_bound(n) and rel_loss <= R.mse_bound(n)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad       # (e)
    assert not parts["per_sample"].requires_grad and not parts["prediction"].requires_grad


@pytest.mark.parametrize("loss_on_first_frame", [False, True])
def test_trainer_matches_the_restatement(tiny, tables, loss_on_first_frame):
    trainer = tiny.trainer(loss_on_first_frame=loss_on_first_frame)
    loss, parts = tiny.forward(trainer)
    _check_against_restatement(trainer, loss, parts, tables)
    assert torch.equal(parts["timesteps"].cpu(), torch.tensor(TIMESTEPS))
    assert torch.equal(_bits(tiny.forward(trainer)[0]), _bits(loss))                     # seeded: the same bits again
    plain = trainer(tiny.videos, tiny.audios, tiny.text, timesteps=torch.tensor(TIMESTEPS), generator=torch.Generator().manual_seed(17))
    assert torch.is_tensor(plain) and torch.equal(_bits(plain), _bits(loss))


@pytest.mark.parametrize("mode,tol", [("bf16", 3e-2), ("fp16", 5e-3)])
def test_trainer_loss_against_the_fp32_unet_oracle(tiny, mode, tol):
    from asva_amd import precision
    from oracle.unet_ref import unet_forward

    precision.set_precision(mode)
    try:
        trainer = tiny.trainer(f32_residual=mode == "fp16")
        loss, parts = tiny.forward(trainer)
        torch.cuda.synchronize()
        per = parts["per_sample"].double().cpu()
    finally:
        precision.set_precision("bf16")
    inputs_noisy, noise, ts = parts["noisy_latents"].cpu(), parts["noise"].cpu(), parts["timesteps"].cpu()
    prep = parts["inputs"]
    n = 4 * 3 * 64
    for b in range(2):
        ref = unet_forward(tiny.sd, tiny.g["config"], inputs_noisy[b:b + 1], int(ts[b]), prep.text_encodings[b:b + 1].cpu(),
                           prep.audio_encodings[b:b + 1].cpu(), prep.audio_masks[b:b + 1].cpu()).double()
        rms_ref = ((ref - noise[b:b + 1].double())[:, :, 1:] ** 2).mean().sqrt().item()
        slack = tol * ref.norm().item() / n ** 0.5
        got = per[b].sqrt().item()
        print(f"MEASURED trainer {mode} sample {b} t={int(ts[b])}: rms {got:.6f}, fp32 oracle {rms_ref:.6f}, |gap| {abs(got - rms_ref):.3e}, "
              f"allowed {slack:.3e}")
        assert abs(got - rms_ref) <= slack


def test_trainer_training_mode_drops_conditions(tiny):
    base = tiny.trainer()
    zero_audio = tiny.forward(base, audios=torch.zeros_like(tiny.audios))[0]
    null_text = tiny.forward(base, text_encodings=tiny.null_text[None].expand(2, -1, -1).contiguous())[0]
    kept = tiny.forward(base)[0]
    assert kept.item() != zero_audio.item() and kept.item() != null_text.item()          # the conditions matter on this network

    drop_audio = tiny.trainer(audio_cond_drop_prob=1.0).train()
    with pytest.warns(RuntimeWarning, match="no gradients"):
        loss, parts = tiny.forward(drop_audio)
    assert torch.equal(_bits(loss), _bits(zero_audio)) and not loss.requires_grad        # the null-audio encodings were used
    with warnings.catch_warnings(record=True) as seen:                                   # the warning fires once
        warnings.simplefilter("always")
        again = tiny.forward(drop_audio)[0]
    assert not [w for w in seen if "no gradients" in str(w.message)]
    assert torch.equal(_bits(again), _bits(loss))
    assert torch.equal(_bits(tiny.forward(drop_audio.eval())[0]), _bits(kept))           # eval mode keeps everything

    drop_text = tiny.trainer(text_cond_drop_prob=1.0).train()
    with pytest.warns(RuntimeWarning):
        loss = tiny.forward(drop_text)[0]
    assert torch.equal(_bits(loss), _bits(null_text))                                    # the null text was used


LP_TIMESTEPS = [1, 500, 981]


def _profiles(trainer, tiny):
    inputs = trainer.prepare(tiny.videos, tiny.audios, tiny.text, torch.Generator().manual_seed(17))
    noise = torch.randn(inputs.latents.shape, generator=torch.Generator().manual_seed(23)).cuda()
    return inputs, noise, [trainer.loss_profile(inputs, LP_TIMESTEPS, noise=noise, rows_per_forward=r) for r in (1, 2, 8)]


def test_loss_profile_does_not_depend_on_its_packing(tiny):
    """Every rows_per_forward in {1, 2, 8} gives the same bits, and row (t, b) equals denoising_loss at that single timestep with
    the same noise.  This needs the UNet to treat a row on its own whatever its batch and its position in it.  On this network
    the GEMM tile and split-K choice is the same at 1, 2 and 6 rows, and what made a row depend on its position was the rotated K
    walk of the GEMMs: with it the same rows were 2.954e-03 (rows_per_forward = 2) and 2.796e-03 (8) relative away from
    rows_per_forward = 1.  The trainer runs its UNet forwards with the unrotated walk (asva_amd/trainer.py unrotated_k_walk)."""
    trainer = tiny.trainer()
    inputs, noise, profiles = _profiles(trainer, tiny)
    singles = torch.stack([trainer.denoising_loss(inputs, timesteps=torch.tensor([t, t]), noise=noise)[1] for t in LP_TIMESTEPS])
    gap = lambda a, b: ((a.double() - b.double()).abs() / b.double()).max().item()  # noqa: E731
    print(f"MEASURED loss_profile t={LP_TIMESTEPS}: rows_per_forward=1 {profiles[0].tolist()}; largest relative gap to it of "
          f"rows_per_forward=2: {gap(profiles[1], profiles[0]):.3e}, of 8: {gap(profiles[2], profiles[0]):.3e}, "
          f"of denoising_loss at one timestep: {gap(singles, profiles[0]):.3e}")
    assert torch.equal(_bits(profiles[0]), _bits(profiles[1])) and torch.equal(_bits(profiles[0]), _bits(profiles[2]))
    assert torch.equal(_bits(singles), _bits(profiles[0]))


class _RowwiseUNet(torch.nn.Module):
    """stand-in for the UNet that treats every batch row on its own, bit for bit: elementwise in the sample, a per-row scalar from
    the timestep and from each condition"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    device = property(lambda self: self.w.device)
    dtype = property(lambda self: self.w.dtype)

    def forward(self, sample, timestep, encoder_hidden_states, audio_encoder_hidden_states, audio_attention_mask, return_dict=True):
        from asva_amd.unet import UNet3DConditionOutput

        k = (timestep.float() / 1000 + encoder_hidden_states.flatten(1)[:, 3] + audio_encoder_hidden_states.flatten(1)[:, 5]
             + audio_attention_mask.flatten(1).float()[:, 300])
        return UNet3DConditionOutput(sample=torch.sin(sample) * k.view(-1, 1, 1, 1, 1))


def test_loss_profile_packing_with_a_rowwise_network(tiny):
    """What the packing and the two kernels owe on their own: with a network that treats each row on its own, every packing gives
    the same bits, whatever the UNet's kernels do."""
    from asva_amd import ops

    krot = ops._KROT
    trainer = tiny.trainer()
    trainer.unet = _RowwiseUNet().to("cuda")
    inputs, noise, profiles = _profiles(trainer, tiny)
    assert profiles[0].shape == (3, 2) and profiles[0].dtype == torch.float32 and profiles[0].is_cuda
    assert torch.equal(_bits(profiles[0]), _bits(profiles[1])) and torch.equal(_bits(profiles[0]), _bits(profiles[2]))
    singles = torch.stack([trainer.denoising_loss(inputs, timesteps=torch.tensor([t, t]), noise=noise)[1] for t in LP_TIMESTEPS])
    assert torch.equal(_bits(singles), _bits(profiles[0]))
    assert len({v for row in profiles[0].tolist() for v in row}) == 6                    # every (timestep, sample) row is its own
    drawn = trainer.loss_profile(inputs, LP_TIMESTEPS, generator=torch.Generator().manual_seed(23), rows_per_forward=8)
    assert torch.equal(_bits(drawn), _bits(profiles[0]))                                 # one draw, shared by all timesteps
    with pytest.raises(ValueError, match="range"):
        trainer.loss_profile(inputs, [1, 1000], noise=noise)
    assert ops._KROT == krot                                                             # the K-walk setting is restored after every forward


# ---- schedulers ------------------------------------------------------------------------------------------------------------
def test_scheduler_add_noise_on_device_tensors_matches_the_cpu_path():
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler

    gen = torch.Generator().manual_seed(9)
    shape = (4, 4, 3, 5, 6)
    x0, noise, ts = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen), torch.tensor([0, 1, 500, 999])
    for cls in (DDIMScheduler, PNDMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler):
        s = cls()
        a, sg = R.coefficients(*R.tables(s.acp), ts)
        for name, velocity in (("add_noise", False), ("get_velocity", True)):
            cpu = getattr(s, name)(x0, noise, ts)
            dev = getattr(s, name)(x0.cuda(), noise.cuda(), ts.cuda())
            assert dev.is_cuda and dev.dtype == torch.float32
            bound = R.elementwise_bound(x0, noise, a, sg, velocity=velocity)
            exact = R.get_velocity(x0, noise, a, sg) if velocity else R.add_noise(x0, noise, a, sg)
            assert bool(((dev.double().cpu() - exact).abs() <= bound).all())
            assert bool(((dev.cpu().double() - cpu.double()).abs() <= bound).all())
    with pytest.raises(ValueError, match="range"):
        PNDMScheduler().add_noise(x0.cuda(), noise.cuda(), torch.tensor([0, 1, 500, 1000]))
