"""DenoiseEngine — the denoising loop of the reference pipeline
(AudioCondAnimationPipeline.__call__, pipeline_audio_cond_animation.py:325-365) as the MI355X hot path:

  per step:  latents --(replicated k times in the layout kernel)--> UNet forward --> noise_pred
             guidance combine + multistep scheduler update + first-frame pinning in ONE kernel
  per clip:  conditioning K/V, position tables and the mask gather list computed once (set_conditioning)

The UNet forward of one step (~650 kernel launches) is captured once into a hipGraph and replayed, so the
host contributes one graph launch + one tiny launch per step instead of ~650 ctypes calls.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


class DenoiseEngine:
    def __init__(self, unet, scheduler, audio_guidance_scale: float = 4.0, text_guidance_scale: float = 1.0,
                 use_graph: bool = True):
        self.unet = unet
        self.scheduler = scheduler
        # guidance mixes of the reference (pipeline_audio_cond_animation.py:349-361), as avsd_guided_step's (n_branch, g, g2):
        #   dual   [uncond, text, text+audio]: e0 + tg (e1 - e0) + ag (e2 - e1)
        #   text   [null-text+audio, text+audio]: e0 + tg (e1 - e0)
        #   audio  [text+null-audio, text+audio]: e0 + ag (e1 - e0)
        self.do_text = text_guidance_scale > 1.0
        self.do_audio = audio_guidance_scale > 1.0
        self.n_branch = 1 + int(self.do_text) + int(self.do_audio)
        if self.do_text and self.do_audio:
            self.g, self.g2 = float(text_guidance_scale), float(audio_guidance_scale)
        elif self.do_text:
            self.g, self.g2 = float(text_guidance_scale), 0.0
        else:
            self.g, self.g2 = float(audio_guidance_scale), 0.0
        # hipGraph replay needs a real device stream (the CPU contract emulation of the tests has none)
        self.use_graph = use_graph and torch.cuda.is_available() and not getattr(ops, "EMULATED", False)
        self._graph = None
        self._graph_key = None
        self.captures = 0      # hipGraphs built so far: stays 1 while clips (or the windows of a track) keep one geometry

    # -- once per clip ---------------------------------------------------------------------------------
    def set_conditioning(self, text: torch.Tensor, audio: torch.Tensor, null_audio: Optional[torch.Tensor],
                         audio_mask: torch.Tensor, video_length: int, null_text: Optional[torch.Tensor] = None):
        """text (b, 77, D); audio (b, 229, D); null_audio (1 or b, 229, D) = encoding of the all-zero
        mel-spectrogram (pipeline :180-184); null_text (1 or b, 77, D) = encoding of "" (:124-148); mask (F, 229).
        Builds the CFG batch exactly as encode_text / encode_audio do (:150-155, :186-194):
        audio-only  text [t, t]      audio [null, a];   text-only  text [null, t]  audio [a, a];
        dual        text [null, t, t]  audio [null, null, a]."""
        b = text.shape[0]
        if self.do_audio:
            if null_audio is None:
                raise ValueError("audio guidance needs the null-audio encoding")
            null_audio = null_audio.expand(b, *null_audio.shape[1:])
        if self.do_text:
            if null_text is None:
                raise ValueError("text guidance needs the null-text encoding")
            null_text = null_text.expand(b, *null_text.shape[1:])
        if self.do_text and self.do_audio:
            text, audio = torch.cat([null_text, text, text], 0), torch.cat([null_audio, null_audio, audio], 0)
        elif self.do_text:
            text, audio = torch.cat([null_text, text], 0), torch.cat([audio, audio], 0)
        elif self.do_audio:
            text, audio = torch.cat([text, text], 0), torch.cat([null_audio, audio], 0)
        self.unet.set_conditioning(text, audio, audio_mask, video_length)

    # -- hot loop -----------------------------------------------------------------------------------------
    def _capture(self, latents: torch.Tensor):
        # the graph bakes in the addresses of the conditioning cache: re-capture only when that was re-allocated
        # (new geometry); same-shape clips refresh it in place (AudioUNet3DConditionModel.set_conditioning)
        key = (tuple(latents.shape), latents.device, self.unet._cond.version, id(self.unet._packed),
               tuple(sorted(getattr(self.unet._cond, "share", {}).items())))   # launch sequence depends on the shared prefix
        if self._graph is not None and self._graph_key == key:
            return
        self._x_static = torch.zeros_like(latents)
        self._t_static = torch.zeros(1, dtype=torch.float32, device=latents.device)
        # warm-up on a side stream (allocator + lazy module loading), then capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.unet.denoise_forward(self._x_static, self._t_static, rep=self.n_branch)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._noise_static = self.unet.denoise_forward(self._x_static, self._t_static, rep=self.n_branch)
        self._graph, self._graph_key = g, key
        self.captures += 1

    def unet_step(self, latents: torch.Tensor, t_dev: torch.Tensor) -> torch.Tensor:
        """noise prediction for the CFG batch; t_dev is a 1-element device f32 tensor."""
        if not self.use_graph:
            return self.unet.denoise_forward(latents, t_dev, rep=self.n_branch)
        self._capture(latents)
        ops.copy(latents, self._x_static)
        self._t_static.copy_(t_dev)
        self._graph.replay()
        return self._noise_static

    def prepare(self, latents: torch.Tensor, num_inference_steps: int, generator=None):
        """`generator`: the DeviceGenerator of a stochastic sampler's noise (DDIM eta > 0, SDE-DPM-Solver++).  Each call takes one
        fresh stream per batch row from it; step i of row b then evaluates the normals (seed, stream0 + b, i) inside its launch
        (schedulers.NoisyStepPlan / NoisyMultistepPlan).  Deterministic samplers take none and leave it untouched."""
        dev = latents.device
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        plans = [self.scheduler.plan_step(i) for i in range(self.scheduler.num_forwards())]
        self._noise_key = None
        if any(getattr(p, "noisy", False) for p in plans):
            from .rng import DeviceGenerator

            if not isinstance(generator, DeviceGenerator):
                raise ValueError(f"{type(self.scheduler).__name__} is stochastic here: prepare() / run() need generator=DeviceGenerator(seed), "
                                 f"got {type(generator).__name__}")
            self._noise_key = (generator.seed, generator.take_streams(latents.shape[0]))
        self._ts = self.scheduler.timesteps.to(dev, torch.float32)
        self._plans = plans
        self._hist = torch.zeros((4,) + tuple(latents.shape), dtype=torch.float32, device=dev)
        self._saved = torch.empty_like(latents)
        self._x_last = torch.zeros_like(latents)       # UniPC: the corrected sample, base of the next step's corrector

    def step(self, latents: torch.Tensor, i: int) -> None:
        """One denoising step in place on `latents` (b, 4, F, H, W) f32: UNet on the CFG batch, then the guidance mix
        (see __init__), scheduler update of frames 1.., frame 0 untouched: the step's plan launches its own kernel (schedulers.py)."""
        noise = self.unet_step(latents, self._ts[i:i + 1])
        self._plans[i].launch(ops, noise, self.n_branch, self.g, self.g2, latents, self)

    @torch.no_grad()
    def run(self, latents: torch.Tensor, num_inference_steps: int, generator=None) -> torch.Tensor:
        latents = latents.to(torch.float32).contiguous().clone()
        self.prepare(latents, num_inference_steps, generator)
        for i in range(len(self._plans)):
            self.step(latents, i)
        return latents
