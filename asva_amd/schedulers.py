"""PNDM (PLMS) and DDIM schedulers for the denoising loop — host-side scalar schedule + one fused device
kernel per step (avsd_guided_step: guidance combine, multistep blend, latent update, frame-0 pinning).

The reference takes its scheduler from diffusers (PNDMScheduler.from_pretrained(sd15, "scheduler"),
pipeline_audio_cond_animation.py:511; called at :325-327,337,364).  diffusers 0.29.2 is not vendored in the
reference nor installed here, so the update rules are restated from its published algorithm
(`PNDMScheduler.set_timesteps/step_plms/_get_prev_sample`, `DDIMScheduler.set_timesteps/step`) for the SD1.5
scheduler_config.json: scaled_linear betas 0.00085..0.012 over 1000 steps, steps_offset 1, skip_prk_steps
true, set_alpha_to_one false, epsilon prediction, "leading" timestep spacing.

Both classes also expose the object protocol the reference pipeline uses (`set_timesteps`, `timesteps`,
`init_noise_sigma`, `scale_model_input`, `step(...).prev_sample`) so they drop into
AudioCondAnimationPipeline; the fast path (`plan_step` + `ops.guided_step`) folds guidance and the update
into one launch and keeps the eps history on the device.

DPMSolverMultistepScheduler (DPM-Solver++ 1M / 2M / 3M, restated from diffusers 0.29.2 the same way) offers the same two
forms; its fast path is `plan_step` + `ops.guided_multistep` (avsd_guided_multistep), whose ring holds data predictions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch


def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, schedule="scaled_linear") -> np.ndarray:
    if schedule == "scaled_linear":
        # diffusers computes this in float32 torch; keep f32 so table entries are bit-identical
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    elif schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    else:
        raise NotImplementedError(schedule)
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


@dataclass
class StepPlan:
    """Everything avsd_guided_step needs for one scheduler step."""
    ca: float                 # coefficient of the (possibly saved) sample
    cb: float                 # coefficient of the blended epsilon
    w_cur: float = 1.0        # weight of this step's epsilon
    store_slot: int = -1      # ring slot to store this step's epsilon in (-1: do not store)
    hist_idx: Tuple[int, ...] = ()
    hist_w: Tuple[float, ...] = ()
    use_saved_sample: bool = False    # PLMS second step restarts from the sample saved at step 0
    save_sample: bool = False         # PLMS first step saves its input sample


@dataclass
class MultistepPlan:
    """Everything avsd_guided_multistep needs for one scheduler step (DPM-Solver++): this step's data prediction is
    d = s_x * x + s_e * eps, and x' = ca * x + c_cur * d + sum_k hist_w[k] * hist[hist_idx[k]]."""
    ca: float                 # coefficient of the sample
    c_cur: float              # coefficient of this step's data prediction
    s_x: float                # d = s_x * x + s_e * eps: 1 / alpha_t and -sigma_t / alpha_t
    s_e: float
    store_slot: int = -1      # ring slot to store d in (-1: do not store)
    hist_idx: Tuple[int, ...] = ()
    hist_w: Tuple[float, ...] = ()


class _Output:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


def _read_config(path: str, subfolder: Optional[str]) -> dict:
    import json
    import os

    p = os.path.join(path, subfolder) if subfolder else path
    with open(os.path.join(p, "scheduler_config.json")) as f:
        cfg = json.load(f)
    return {k: v for k, v in cfg.items() if not k.startswith("_")}


class _Base:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 steps_offset=1, set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading",
                 trained_betas=None, clip_sample=False, thresholding=False, rescale_betas_zero_snr=False, **unknown):
        if prediction_type != "epsilon" or timestep_spacing != "leading":
            raise NotImplementedError("only the SD1.5 scheduler configuration (epsilon, leading) is restated")
        # options that change the samples must not be dropped silently (diffusers' DDIM default is clip_sample=True;
        # the SD1.5 scheduler_config.json sets it to false)
        if clip_sample or thresholding or rescale_betas_zero_snr or trained_betas is not None:
            raise NotImplementedError("clip_sample / thresholding / rescale_betas_zero_snr / trained_betas are not restated: "
                                      "the SD1.5 scheduler configuration sets none of them")
        known_inert = {"clip_sample_range", "dynamic_thresholding_ratio", "sample_max_value", "skip_prk_steps"}
        bad = sorted(k for k in unknown if not k.startswith("_") and k not in known_inert)
        if bad:
            raise NotImplementedError(f"unknown scheduler options {bad}")
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.acp = alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.acp[0])
        self.num_inference_steps: Optional[int] = None
        self.timesteps: Optional[torch.Tensor] = None
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, steps_offset=steps_offset, set_alpha_to_one=set_alpha_to_one,
                           prediction_type=prediction_type, timestep_spacing=timestep_spacing)

    def scale_model_input(self, sample, timestep=None):
        return sample

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None):
        return cls(**_read_config(path, subfolder))

    def _acp(self, t: int) -> float:
        return float(self.acp[t]) if t >= 0 else self.final_alpha_cumprod


class DDIMScheduler(_Base):
    """eta = 0, no clipping / thresholding: x' = sqrt(a'/a) x + (sqrt(1-a') - sqrt(a'(1-a)/a)) eps."""

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self._ts = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def num_forwards(self) -> int:
        return len(self._ts)

    def plan_step(self, i: int) -> StepPlan:
        t = self._ts[i]
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a, ap = self._acp(t), self._acp(prev)
        ca = (ap / a) ** 0.5
        cb = (1.0 - ap) ** 0.5 - (ap * (1.0 - a) / a) ** 0.5
        return StepPlan(ca=ca, cb=cb)

    def step(self, model_output, timestep, sample, eta: float = 0.0, generator=None, return_dict=True, **_):
        if eta != 0.0:
            raise NotImplementedError("DDIM eta != 0")
        i = self._ts.index(int(timestep))
        p = self.plan_step(i)
        prev = p.ca * sample + p.cb * model_output
        return _Output(prev) if return_dict else (prev,)


class PNDMScheduler(_Base):
    """PLMS (skip_prk_steps=True): 4th-order linear multistep on the stored epsilons, with the doubled second
    timestep that bootstraps the history (diffusers step_plms)."""

    ring_slots = 4

    def __init__(self, skip_prk_steps=True, cur_sample_aliases_latents: bool = True, **kw):
        """cur_sample_aliases_latents (default True = what the reference pipeline actually computes): diffusers'
        step_plms keeps `self.cur_sample = sample` WITHOUT cloning, and the reference passes a view,
        `video_latents[:, :, 1:]`, then writes the result back into that same storage
        (pipeline_audio_cond_animation.py:364; `.contiguous()` on :365 is a no-op).  The sample "restored" at the
        repeated second timestep is therefore the already-updated latents x1, not x0.  False gives textbook PLMS
        (what diffusers does when the caller rebinds `latents = step(...).prev_sample`)."""
        super().__init__(**kw)
        if not skip_prk_steps:
            raise NotImplementedError("PRK warm-up steps (skip_prk_steps=False)")
        self.config["skip_prk_steps"] = True
        self.cur_sample_aliases_latents = cur_sample_aliases_latents

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        base = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.steps_offset
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        self._ts = [int(t) for t in plms]
        self.timesteps = torch.from_numpy(plms).to(device) if device is not None else torch.from_numpy(plms)
        # object-protocol state
        self.ets: List[torch.Tensor] = []
        self.counter = 0
        self.cur_sample = None

    def num_forwards(self) -> int:
        return len(self._ts)

    def _coeffs(self, t: int, prev: int) -> Tuple[float, float]:
        a, ap = self._acp(t), self._acp(prev)
        b, bp = 1.0 - a, 1.0 - ap
        ca = (ap / a) ** 0.5
        denom = a * bp ** 0.5 + (a * b * ap) ** 0.5
        return ca, -(ap - a) / denom

    def plan_step(self, i: int) -> StepPlan:
        """Step i of the loop (i = diffusers' `counter`).  History ring: epsilon of the k-th APPENDING step
        lives in slot k % 4; step 1 (the repeated timestep) does not append."""
        ratio = self.num_train_timesteps // self.num_inference_steps
        t = self._ts[i]
        prev = t - ratio
        if i == 1:
            prev, t = t, t + ratio
        ca, cb = self._coeffs(t, prev)
        textbook = not self.cur_sample_aliases_latents
        if i == 0:
            return StepPlan(ca, cb, w_cur=1.0, store_slot=0, save_sample=textbook)
        if i == 1:
            return StepPlan(ca, cb, w_cur=0.5, store_slot=-1, hist_idx=(0,), hist_w=(0.5,), use_saved_sample=textbook)
        n_app = i            # appended epsilons after this step's append: steps 0,2,3,... -> i of them (i >= 2)
        cur = (n_app - 1) % self.ring_slots
        s = lambda back: (n_app - 1 - back) % self.ring_slots  # noqa: E731
        if n_app == 2:
            return StepPlan(ca, cb, 0.0, cur, (s(0), s(1)), (1.5, -0.5))
        if n_app == 3:
            return StepPlan(ca, cb, 0.0, cur, (s(0), s(1), s(2)), (23 / 12, -16 / 12, 5 / 12))
        return StepPlan(ca, cb, 0.0, cur, (s(0), s(1), s(2), s(3)), (55 / 24, -59 / 24, 37 / 24, -9 / 24))

    # object protocol (tensor-level, any device) — the same arithmetic, used when the scheduler is driven
    # through `.step()` by the reference-style loop.  Like diffusers it keeps `sample` itself (no clone), so a
    # caller that passes a view and writes back in place gets the aliasing described in __init__.
    def step(self, model_output, timestep, sample, return_dict=True, **_):
        ratio = self.num_train_timesteps // self.num_inference_steps
        t = int(timestep)
        prev = t - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev, t = t, t + ratio
        if len(self.ets) == 1 and self.counter == 0:
            # diffusers keeps the caller's tensor itself (no clone): see __init__ for what that means for a caller that
            # writes the result back into the same storage.  Textbook PLMS keeps a copy.
            self.cur_sample = sample if self.cur_sample_aliases_latents else sample.clone()
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])
        ca, cb = self._coeffs(t, prev)
        prev_sample = ca * sample + cb * model_output
        self.counter += 1
        return _Output(prev_sample) if return_dict else (prev_sample,)


class DPMSolverMultistepScheduler:
    """DPM-Solver++ (Lu et al. 2022, arXiv:2211.01095), multistep, orders 1-3, restated from diffusers 0.29.2's
    `DPMSolverMultistepScheduler` (`set_timesteps`, `convert_model_output`, `dpm_solver_first_order_update`,
    `multistep_dpm_solver_second_order_update`, `multistep_dpm_solver_third_order_update`, `step`) for the deterministic
    data-prediction solver on an epsilon-predicting model.

    With sigma = sqrt((1 - acp) / acp), alpha_t = 1 / sqrt(1 + sigma^2), sigma_t = sigma * alpha_t and
    lambda = log(alpha_t) - log(sigma_t), step i turns eps into the data prediction x0 = (x - sigma_t eps) / alpha_t and moves x
    from sigmas[i] to sigmas[i + 1] with the exponential-integrator update of order 1, 2 or 3 over the last x0s.

    The fast path (`plan_step` + `ops.guided_multistep`) keeps the last x0s in the engine's 4-slot ring (step i stores its x0
    in slot i % solver_order) and folds guidance, x0 and the update into one launch; its coefficients are computed on the host
    in float64.

    Choices that cannot be checked here (diffusers is absent):
      * the solver options default to diffusers' values, but the beta schedule defaults to SD1.5's (scaled_linear
        0.00085..0.012), as PNDMScheduler / DDIMScheduler here do; diffusers' own constructor default is linear 0.0001..0.02.
        `from_pretrained` / `from_config` take whatever the configuration says.
      * diffusers evaluates a step's scalars (alpha_t, sigma_t, lambda, h) as float32 tensors; here they are float64 from the
        float32 sigma table, so a coefficient may differ from diffusers' in its last float32 bit.
      * the last step is first order when final_sigmas_type is "zero" (h is infinite there) or when lower_order_final is set
        and there are fewer than 15 steps; in the latter case the second-to-last step is at most second order.
      * Karras sigmas end on sigma_min, so with final_sigmas_type="sigma_min" the last step has h = 0; here it leaves x
        unchanged at every order (diffusers' midpoint update does the same; its heun and third-order updates divide by h).
      * the third-order update is the published one (D2 = (D1_0 - D1_1) / (r0 + r1) times -alpha_t phi_3).  It weighs the
        second-derivative term at half of a third-order Taylor match, so on an exactly solvable problem 3M converges at order 2,
        with a smaller constant than 2M (tests/test_dpmsolver_cpu.py measures both).
    Every other option that changes the samples (SDE variants, thresholding, v- / sample prediction, variance_type,
    euler_at_final, lambda_min_clipped, Lu lambdas, rescale_betas_zero_snr, trained_betas) raises NotImplementedError.
    """

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero",
                 lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
                 rescale_betas_zero_snr=False, **unknown):
        if algorithm_type != "dpmsolver++" or prediction_type != "epsilon":
            raise NotImplementedError("only algorithm_type='dpmsolver++' with prediction_type='epsilon' is restated")
        if solver_order not in (1, 2, 3) or solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_order {solver_order!r} / solver_type {solver_type!r}: orders 1-3, midpoint or heun")
        if final_sigmas_type not in ("zero", "sigma_min") or timestep_spacing not in ("linspace", "leading", "trailing"):
            raise NotImplementedError(f"final_sigmas_type {final_sigmas_type!r} / timestep_spacing {timestep_spacing!r}")
        if (thresholding or euler_at_final or use_lu_lambdas or variance_type is not None or rescale_betas_zero_snr
                or trained_betas is not None or lambda_min_clipped != -float("inf")):
            raise NotImplementedError("thresholding / euler_at_final / use_lu_lambdas / variance_type / lambda_min_clipped / "
                                      "rescale_betas_zero_snr / trained_betas are not restated")
        # keys of the SD1.5 PNDM / DDIM configurations that DPM-Solver++ does not have (diffusers ignores them as well)
        known_inert = {"skip_prk_steps", "set_alpha_to_one", "clip_sample", "clip_sample_range"}
        bad = sorted(k for k in unknown if not k.startswith("_") and k not in known_inert)
        if bad:
            raise NotImplementedError(f"unknown scheduler options {bad}")
        self.num_train_timesteps = num_train_timesteps
        self.solver_order, self.solver_type, self.lower_order_final = solver_order, solver_type, lower_order_final
        self.final_sigmas_type, self.use_karras_sigmas = final_sigmas_type, use_karras_sigmas
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset
        self.acp = alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.num_inference_steps: Optional[int] = None
        self.timesteps: Optional[torch.Tensor] = None
        self.sigmas: Optional[np.ndarray] = None
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                           algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                           use_karras_sigmas=use_karras_sigmas, final_sigmas_type=final_sigmas_type,
                           timestep_spacing=timestep_spacing, steps_offset=steps_offset)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None):
        return cls(**_read_config(path, subfolder))

    @classmethod
    def from_config(cls, config, **overrides):
        """diffusers' `DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: another scheduler's configuration,
        with its own keys (PNDM's skip_prk_steps, ...) accepted and ignored."""
        return cls(**{k: v for k, v in {**dict(config), **overrides}.items() if not k.startswith("_")})

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps: int, device=None):
        n, T = num_inference_steps, self.num_train_timesteps
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        else:
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1
        train = ((1.0 - self.acp) / self.acp) ** 0.5
        if self.use_karras_sigmas:
            # Karras et al. 2022 (eq. 5, rho = 7) from the schedule's sigma_max down to its sigma_min; timesteps interpolated in log sigma
            rho, lo, hi = 7.0, train[0], train[-1]
            sig = (hi ** (1 / rho) + np.linspace(0, 1, n) * (lo ** (1 / rho) - hi ** (1 / rho))) ** rho
            ts = self._sigma_to_t(sig, np.log(train)).round().astype(np.int64)
        else:
            sig = np.interp(ts, np.arange(len(train)), train)
        last = train[0] if self.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = np.concatenate([sig, [last]]).astype(np.float32).astype(np.float64)    # diffusers keeps the table in float32
        self._ts = [int(t) for t in ts]
        self.num_inference_steps = len(self._ts)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        # object-protocol state
        self.model_outputs: List[Optional[torch.Tensor]] = [None] * self.solver_order
        self.lower_order_nums = 0
        self._step_index: Optional[int] = None

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        low = np.cumsum(log_sigma - log_sigmas[:, None] >= 0, axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        lo, hi = log_sigmas[low], log_sigmas[low + 1]
        w = np.clip((lo - log_sigma) / (lo - hi), 0, 1)
        return (1 - w) * low + w * (low + 1)

    def num_forwards(self) -> int:
        return len(self._ts)

    @staticmethod
    def _alpha_sigma(sigma: float) -> Tuple[float, float]:
        alpha_t = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return alpha_t, sigma * alpha_t

    def _lambda(self, i: int) -> float:
        alpha_t, sigma_t = self._alpha_sigma(float(self.sigmas[i]))
        return math.log(alpha_t) - math.log(sigma_t)

    def _coeffs(self, i: int):
        """x' = ca x + c0 D0 + c1 D1 + c2 D2 for the step sigmas[i] -> sigmas[i + 1], and the ratios r0 = h_0 / h, r1 = h_1 / h of
        the previous two steps' lambda increments to this one's (None where there is no such step)"""
        alpha_t, sigma_t = self._alpha_sigma(float(self.sigmas[i + 1]))
        sigma_s0 = self._alpha_sigma(float(self.sigmas[i]))[1]
        if sigma_t == 0.0:       # final sigma zero: h is infinite, the first-order update returns the data prediction itself
            return 0.0, alpha_t, None, None, None, None
        h = self._lambda(i + 1) - self._lambda(i)
        if h == 0.0:             # Karras sigmas end on sigma_min: with final_sigmas_type="sigma_min" the last step does not move x
            return 1.0, 0.0, None, None, None, None
        em = math.exp(-h) - 1.0
        c1 = alpha_t * (em / h + 1.0)
        c2 = -alpha_t * ((em + h) / (h * h) - 0.5)
        r0 = (self._lambda(i) - self._lambda(i - 1)) / h if i >= 1 else None
        r1 = (self._lambda(i - 1) - self._lambda(i - 2)) / h if i >= 2 else None
        return sigma_t / sigma_s0, -alpha_t * em, c1, c2, r0, r1

    def _lower_order(self, i: int) -> Tuple[bool, bool]:
        n = len(self._ts)
        few = self.lower_order_final and n < 15
        return i == n - 1 and (few or self.final_sigmas_type == "zero"), i == n - 2 and few

    def plan_step(self, i: int) -> MultistepPlan:
        """Step i as coefficients of avsd_guided_multistep.  The data prediction of step j lives in ring slot j % solver_order;
        it is stored only when a later step reads it."""
        last_first, second_last = self._lower_order(i)
        alpha_s, sigma_s = self._alpha_sigma(float(self.sigmas[i]))
        ca, c0, c1, c2, r0, r1 = self._coeffs(i)
        if self.solver_order == 1 or i < 1 or last_first or c1 is None:
            k = 1
        elif self.solver_order == 2 or i < 2 or second_last:
            k = 2
        else:
            k = 3
        slot = lambda j: j % self.solver_order  # noqa: E731
        store = slot(i) if self.solver_order > 1 and i < len(self._ts) - 1 else -1
        if k == 1:
            cur, idx, w = c0, (), ()
        elif k == 2:
            cd = (0.5 * c0 if self.solver_type == "midpoint" else c1) / r0      # D1 = (m0 - m1) / r0
            cur, idx, w = c0 + cd, (slot(i - 1),), (-cd,)
        else:
            # D1 = (1 + q) a m0 - ((1 + q) a + q b) m1 + q b m2,  D2 = p (a m0 - (a + b) m1 + b m2)
            a, b, q, p = 1.0 / r0, 1.0 / r1, r0 / (r0 + r1), 1.0 / (r0 + r1)
            cur = c0 + c1 * (1 + q) * a + c2 * p * a
            idx = (slot(i - 1), slot(i - 2))
            w = (-c1 * ((1 + q) * a + q * b) - c2 * p * (a + b), c1 * q * b + c2 * p * b)
        return MultistepPlan(ca=ca, c_cur=cur, s_x=1.0 / alpha_s, s_e=-sigma_s / alpha_s, store_slot=store, hist_idx=idx, hist_w=w)

    # object protocol (tensor-level, any device): diffusers' step, written over the data predictions themselves
    def step(self, model_output, timestep, sample, return_dict=True, **_):
        if self._step_index is None:
            hits = [j for j, t in enumerate(self._ts) if t == int(timestep)]
            self._step_index = (hits[1] if len(hits) > 1 else hits[0]) if hits else len(self._ts) - 1
        i = self._step_index
        last_first, second_last = self._lower_order(i)
        alpha_s, sigma_s = self._alpha_sigma(float(self.sigmas[i]))
        x0 = (sample - sigma_s * model_output) / alpha_s
        self.model_outputs = self.model_outputs[1:] + [x0]
        m = self.model_outputs
        ca, c0, c1, c2, r0, r1 = self._coeffs(i)
        if self.solver_order == 1 or self.lower_order_nums < 1 or last_first or c1 is None:
            prev_sample = ca * sample + c0 * x0
        elif self.solver_order == 2 or self.lower_order_nums < 2 or second_last:
            D1 = (1.0 / r0) * (m[-1] - m[-2])
            prev_sample = ca * sample + c0 * m[-1] + (0.5 * c0 if self.solver_type == "midpoint" else c1) * D1
        else:
            D1_0, D1_1 = (1.0 / r0) * (m[-1] - m[-2]), (1.0 / r1) * (m[-2] - m[-3])
            D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
            D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
            prev_sample = ca * sample + c0 * m[-1] + c1 * D1 + c2 * D2
        self.lower_order_nums = min(self.lower_order_nums + 1, self.solver_order)
        self._step_index += 1
        return _Output(prev_sample) if return_dict else (prev_sample,)
