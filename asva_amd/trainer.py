"""AudioCondAnimationTrainer: the denoising loss the network was trained on, forward value only, on the device.

Reference: avgen/models/trainers/audio_cond_animation_trainer.py.  Its `forward` encodes the clip to latents, draws one timestep
and one noise tensor per sample, noises frames 1.. (frame 0 stays clean), runs the UNet once and takes the mean squared error
against the noise.  Here the noising step is one avsd_diffuse_clip_f32 launch, the UNet is AudioUNet3DConditionModel.forward with
one timestep per batch row, and the reduction is avsd_frame_mse_f32 (deterministic, per-sample values as well as their mean).

`forward` is split so that the timestep-independent part (VAE encode, audio encoder, condition dropping) runs once:
`prepare` -> TrainerInputs, then `denoising_loss` / `loss_profile` on those inputs as often as wanted.

The random stream is not the reference's: it draws the timesteps on the CPU and the noise with the global device generator.
Pass `timesteps=` / `noise=` to compare the two on equal inputs.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import ops

NULL_TEXT_ENCODING_PATH = "pretrained/openai-clip-l_null_text_encoding.pt"     # the reference's hard-coded file


def prob_mask_like(shape, prob: float, device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The reference's rule: all True at prob 1, all False at prob 0, otherwise uniform(0, 1) < prob."""
    if prob == 1:
        return torch.ones(shape, device=device, dtype=torch.bool)
    if prob == 0:
        return torch.zeros(shape, device=device, dtype=torch.bool)
    return _draw(torch.rand, shape, generator, device) < prob


def keep_masks(batch: int, training: bool, text_cond_drop_prob: float, audio_cond_drop_prob: float, device,
               generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(text keep mask, audio keep mask), (batch,) bool each: drawn with prob_mask_like in training mode, all True otherwise."""
    if not training:
        return prob_mask_like((batch,), 1.0, device), prob_mask_like((batch,), 1.0, device)
    return (prob_mask_like((batch,), 1 - text_cond_drop_prob, device, generator),
            prob_mask_like((batch,), 1 - audio_cond_drop_prob, device, generator))


def pack_rows(n_timesteps: int, batch: int, rows_per_forward: int) -> List[List[Tuple[int, int]]]:
    """loss_profile's packing: every (timestep index, sample index) pair exactly once, timestep-major, in UNet batches of at most
    `rows_per_forward` rows."""
    if n_timesteps < 0 or batch <= 0 or rows_per_forward <= 0:
        raise ValueError("pack_rows: need n_timesteps >= 0, batch > 0 and rows_per_forward > 0")
    pairs = [(ti, bi) for ti in range(n_timesteps) for bi in range(batch)]
    return [pairs[i:i + rows_per_forward] for i in range(0, len(pairs), rows_per_forward)]


def _draw(fn, shape, generator, device, **kw):
    """fn(shape, generator=...) on the generator's own device (a CPU generator cannot fill a device tensor), moved to `device`"""
    where = generator.device if generator is not None else device
    return fn(tuple(shape), generator=generator, device=where, **kw).to(device)


@contextlib.contextmanager
def unrotated_k_walk():
    """The UNet forwards of the trainer run with the GEMMs' unrotated K walk (ops.set_krot(False)).  With the rotated walk a row
    band starts its K loop at a tile that depends on the band's index, so the f32 summation order of a row, and with it the 16-bit
    rounding of every activation behind it, follows the row's POSITION in the batch: the same sample then gives a loss 3e-3 apart
    in another packing of loss_profile (measured on the tiny test network).  Unrotated, every tile of a family sums K in one order.
    The rotation is worth about 2 % of a denoising step (asva_amd/ops.py) and nothing to a loss; the setting is restored on exit."""
    before = ops._KROT
    ops.set_krot(False)
    try:
        yield
    finally:
        ops.set_krot(before)


def _cfg(scheduler, key: str):
    c = scheduler.config
    return c[key] if isinstance(c, dict) else getattr(c, key)


@dataclass
class TrainerInputs:
    """What the reference's forward has computed before it draws timesteps (steps 1-2)."""
    latents: torch.Tensor               # (b, C, f, h, w) f32: latent_dist.sample() * scaling_factor
    text_encodings: torch.Tensor        # (b, f, L, D): null text where the keep mask dropped the sample
    audio_encodings: torch.Tensor       # (b, f, n, c): null-audio encodings where dropped
    audio_masks: torch.Tensor           # (b, f, n) bool
    text_keep: torch.Tensor             # (b,) bool
    audio_keep: torch.Tensor            # (b,) bool


class AudioCondAnimationTrainer(nn.Module):
    """Device counterpart of the reference's AudioCondAnimationTrainer, for the VALUE of its training objective.

    The result never carries gradients: the VAE, the audio encoder and the UNet run their inference kernels, and no backward pass
    exists here.  `loss.backward()` therefore fails in torch with its own message; calling `forward` in training mode warns once.
    Training mode still matters: it is what turns the condition dropping (`text_cond_drop_prob`, `audio_cond_drop_prob`) on.

    Constructor arguments as in the reference, plus `null_text_encoding`: a tensor (..., L, D) or the path of one, by default the
    reference's hard-coded `pretrained/openai-clip-l_null_text_encoding.pt`.
    """

    def __init__(self, vae, audio_encoder, unet, scheduler, text_cond_drop_prob: float = 0.0, audio_cond_drop_prob: float = 0.0,
                 loss_on_first_frame: bool = False, null_text_encoding: Union[torch.Tensor, str, os.PathLike] = NULL_TEXT_ENCODING_PATH):
        super().__init__()
        self.audio_encoder = audio_encoder
        self.vae = vae
        self.unet = unet
        self.scheduler = scheduler
        self.text_cond_drop_prob = text_cond_drop_prob
        self.audio_cond_drop_prob = audio_cond_drop_prob
        self.loss_on_first_frame = loss_on_first_frame
        if not torch.is_tensor(null_text_encoding):
            path = os.fspath(null_text_encoding)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"null text encoding not found: {path} (pass null_text_encoding= a tensor or another path)")
            null_text_encoding = torch.load(path, map_location="cpu", weights_only=True)
        enc = null_text_encoding.detach().float()
        if enc.dim() < 2:
            raise ValueError(f"null_text_encoding: expected (..., tokens, channels), got {tuple(enc.shape)}")
        enc = enc.reshape(1, 1, -1, enc.shape[-1]) if enc.dim() == 2 else enc.reshape(1, 1, *enc.shape[-2:])
        self.null_text_encoding = nn.Parameter(enc.clone(), requires_grad=False)      # (1, 1, 77, 768) in the reference
        self._warned_training = False

    @property
    def device(self):
        return self.unet.device

    @property
    def dtype(self):
        return self.unet.dtype

    @torch.no_grad()
    def compress_to_latents(self, images: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """images (b, 3, H, W) normalised to [-1, 1] -> latents (b, c, h, w) = latent_dist.sample() * scaling_factor"""
        dist = self.vae.encode(images).latent_dist
        noise = _draw(torch.randn, dist.mean.shape, generator, dist.mean.device, dtype=dist.mean.dtype)
        return dist.sample(noise=noise) * self.vae.config.scaling_factor

    @torch.no_grad()
    def prepare(self, videos: torch.Tensor, audios: torch.Tensor, text_encodings: torch.Tensor,
                generator: Optional[torch.Generator] = None) -> TrainerInputs:
        """Steps 1-2 of the reference's forward.  videos (b, 3, f, H, W) in [0, 1]; audios as the audio encoder takes them;
        text_encodings (b, L, D)."""
        assert videos.ndim == 5, "videos must be in shape (b c f h w) in range [0, 1]"
        b, f = videos.size(0), videos.size(2)
        dev = self.device
        frames = videos.to(dev).permute(0, 2, 1, 3, 4).reshape(b * f, *videos.shape[1:2], *videos.shape[3:])
        latents = self.compress_to_latents((frames.float() - 0.5) / 0.5, generator)
        latents = latents.reshape(b, f, *latents.shape[1:]).permute(0, 2, 1, 3, 4).float().contiguous()

        audios = audios.to(dev)
        _, audio_enc, audio_masks = self.audio_encoder(audios, return_dict=False)
        _, null_enc, null_masks = self.audio_encoder(torch.zeros_like(audios), return_dict=False)

        text_keep, audio_keep = keep_masks(b, self.training, self.text_cond_drop_prob, self.audio_cond_drop_prob, dev, generator)
        text = text_encodings.to(device=dev, dtype=self.dtype)
        null_text = self.null_text_encoding[0].to(device=dev, dtype=self.dtype).expand_as(text).contiguous()
        text = torch.where(text_keep[:, None, None], text, null_text)
        text = text.unsqueeze(1).expand(b, f, *text.shape[1:]).contiguous()
        audio_enc = torch.where(audio_keep[:, None, None], audio_enc, null_enc)
        audio_enc = audio_enc.unsqueeze(1).expand(b, f, *audio_enc.shape[1:]).contiguous().to(self.dtype)
        audio_masks = torch.where(audio_keep[:, None, None], audio_masks, null_masks).contiguous()
        return TrainerInputs(latents, text, audio_enc, audio_masks, text_keep, audio_keep)

    # ---- steps 3-5 -------------------------------------------------------------------------------------------------------
    def _mode(self) -> str:
        kind = _cfg(self.scheduler, "prediction_type")
        if kind not in ("epsilon", "v_prediction"):
            raise ValueError(f"Unknown prediction type {kind}")
        return kind

    def _draw_noise(self, inputs: TrainerInputs, noise, generator) -> torch.Tensor:
        lat = inputs.latents
        if noise is None:
            return _draw(torch.randn, lat.shape, generator, lat.device, dtype=torch.float32)
        if noise.shape != lat.shape:
            raise ValueError(f"noise {tuple(noise.shape)} must have the latents' shape {tuple(lat.shape)}")
        return noise.to(device=lat.device, dtype=torch.float32).contiguous()

    @torch.no_grad()
    def _denoise(self, latents, noise, timesteps, text, audio, masks) -> dict:
        mode = self._mode()
        tab_a, tab_s = self.scheduler.noise_tables(latents.device)
        noisy, target = ops.diffuse_clip(latents, noise, timesteps, tab_a, tab_s, keep_first=True, mode=mode,
                                         want_target=mode != "epsilon")
        ts = timesteps.to(latents.device)
        with unrotated_k_walk():
            pred = self.unet(sample=noisy, timestep=ts, encoder_hidden_states=text, audio_encoder_hidden_states=audio,
                             audio_attention_mask=masks, return_dict=True).sample
        pred = pred.float().contiguous()
        loss, per_sample = ops.frame_mse(pred, noise if target is None else target, 0 if self.loss_on_first_frame else 1)
        return dict(loss=loss, per_sample=per_sample, noisy_latents=noisy, prediction=pred, target=noise if target is None else target)

    def _parts(self, inputs: TrainerInputs, timesteps, noise, generator) -> dict:
        lat = inputs.latents
        if lat.shape[2] - (0 if self.loss_on_first_frame else 1) <= 0:
            raise ValueError("a one-frame clip has no frames to score unless loss_on_first_frame is set")
        T = int(_cfg(self.scheduler, "num_train_timesteps"))
        if timesteps is None:
            timesteps = _draw(lambda size, **kw: torch.randint(0, T, size, **kw), (lat.shape[0],), generator, lat.device)
        timesteps = torch.as_tensor(timesteps)
        noise = self._draw_noise(inputs, noise, generator)
        out = self._denoise(lat, noise, timesteps, inputs.text_encodings, inputs.audio_encodings, inputs.audio_masks)
        out.update(latents=lat, noise=noise, timesteps=timesteps)
        return out

    def denoising_loss(self, inputs: TrainerInputs, timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                       generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Steps 3-5 on prepared inputs -> (loss 0-dim f32, per_sample (b,) f32), on the device.  Draws what is not given:
        timesteps uniform in [0, num_train_timesteps), noise standard normal."""
        out = self._parts(inputs, timesteps, noise, generator)
        return out["loss"], out["per_sample"]

    def forward(self, videos: torch.Tensor, audios: torch.Tensor, text_encodings: torch.Tensor, *, timesteps: Optional[torch.Tensor] = None,
                noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, return_parts: bool = False):
        """`prepare` then `denoising_loss`: the reference's forward.  -> 0-dim f32 device tensor; with return_parts also a dict of
        latents, noise, timesteps, noisy_latents, prediction, target, per_sample and the prepared inputs."""
        if self.training and not self._warned_training:
            self._warned_training = True
            warnings.warn("AudioCondAnimationTrainer computes the forward value only: the loss carries no gradients and "
                          "loss.backward() will fail", RuntimeWarning, stacklevel=2)
        inputs = self.prepare(videos, audios, text_encodings, generator)
        out = self._parts(inputs, timesteps, noise, generator)
        out["inputs"] = inputs
        loss = out.pop("loss")
        return (loss, out) if return_parts else loss

    @torch.no_grad()
    def loss_profile(self, inputs: TrainerInputs, timesteps: Sequence[int], noise: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None, rows_per_forward: int = 8) -> torch.Tensor:
        """Per-sample losses at each of `timesteps` -> (len(timesteps), b) f32 on the device.  One noise draw is shared by all
        timesteps; the (timestep, sample) pairs are packed into UNet batches of at most `rows_per_forward` rows (pack_rows).
        The packing and the two kernels treat a batch row on its own, bit for bit, and so does the UNet as the trainer runs it
        (unrotated_k_walk) wherever the GEMM tile and split-K choice is the same for the row counts involved: on the tiny test
        network every packing gives the same bits (tests/test_trainer_gpu.py).  asva_amd/ops.py chooses tiles by the row count, so
        at shapes where that choice changes between two packings a row still moves in the low bits of the 16-bit activations;
        tools/denoise_loss.py prints that gap for the SD1.5 shape."""
        lat = inputs.latents
        b, dev = lat.shape[0], lat.device
        T = int(_cfg(self.scheduler, "num_train_timesteps"))
        ts_all = ops.check_timesteps(torch.as_tensor(list(timesteps), dtype=torch.int64), len(timesteps), T, "cpu") if len(timesteps) else None
        noise = self._draw_noise(inputs, noise, generator)
        out = torch.empty((len(timesteps), b), dtype=torch.float32, device=dev)
        gathered = {}                      # sample pattern -> gathered rows: equal patterns in a row keep the UNet's conditioning cache
        for chunk in pack_rows(len(timesteps), b, rows_per_forward):
            ti = [p[0] for p in chunk]
            bi = tuple(p[1] for p in chunk)
            if bi not in gathered:
                idx = torch.tensor(bi, device=dev)
                gathered[bi] = tuple(t.index_select(0, idx).contiguous()
                                     for t in (lat, noise, inputs.text_encodings, inputs.audio_encodings, inputs.audio_masks))
            x0, nz, text, audio, masks = gathered[bi]
            per = self._denoise(x0, nz, ts_all[ti], text, audio, masks)["per_sample"]
            out[torch.tensor(ti, device=dev), torch.tensor(bi, device=dev)] = per
        return out

    def save_pretrained(self, directory):
        os.makedirs(directory, exist_ok=True)
        self.unet.save_pretrained(os.path.join(directory, "unet"))
        self.audio_encoder.save_pretrained(os.path.join(directory, "audio_encoder"))
