"""Contracts of the two stochastic step kernels (include/avsd.h: avsd_guided_step_sde, avsd_guided_multistep_sde), computed in the
dtype of their arguments: the deterministic contract (tests/emu_ops.py guided_step, tests/test_dpmsolver_cpu.py guided_multistep)
plus c_noise * z on frames 1.., and the closed forms the CPU tests of the two samplers check the plans against.

The normals are those of tests/philox_ref.py rounded to f32, which is what the device produces and what the emulated
`ops.randn_philox` of tests/test_stochastic_cpu.py returns: batch row b takes `C (F - 1) H W` of them from (seed, stream + b, step)
in the layout (C, F - 1, H, W).  `noise=` replaces them (the GPU tests pass the device's own)."""
import math

import numpy as np
import torch

from tests import emu_ops, philox_ref
from tests.test_dpmsolver_cpu import guided_multistep


def step_noise(shape, seed, stream, step, dtype=torch.float64):
    """(B, C, F - 1, H, W) for latents of `shape` = (B, C, F, H, W)"""
    B, C, F, H, W = shape
    n = C * (F - 1) * H * W
    rows = [torch.from_numpy(philox_ref.normals(n, seed, stream + b, step).astype(np.float32)).reshape(C, F - 1, H, W)
            for b in range(B)] if n else [torch.zeros(C, 0, H, W) for _ in range(B)]
    return torch.stack(rows).to(dtype)


def _add_noise(x_out, c_noise, seed, stream, step, noise):
    if stream + x_out.shape[0] > 1 << 32:
        raise ValueError("stream + B exceeds 2^32")
    z = step_noise(x_out.shape, seed, stream, step, x_out.dtype) if noise is None else noise.to(x_out.dtype)
    x_out[:, :, 1:] += c_noise * z


def guided_step_sde(noise_pred, n_branch, g, x_in, x_out, ca, cb, *, eps_hist=None, store_slot=-1, w_cur=1.0, hist_idx=(), w=(),
                    g2=0.0, c_noise=0.0, seed=0, stream=0, step=0, noise=None):
    emu_ops.guided_step(noise_pred, n_branch, g, x_in, x_out, ca, cb, eps_hist=eps_hist, store_slot=store_slot, w_cur=w_cur,
                        hist_idx=hist_idx, w=w, g2=g2)
    _add_noise(x_out, c_noise, seed, stream, step, noise)


def guided_multistep_sde(noise_pred, n_branch, g, x_in, x_out, ca, c_cur, s_x, s_e, *, hist=None, store_slot=-1, hist_idx=(), w=(),
                         g2=0.0, c_noise=0.0, seed=0, stream=0, step=0, noise=None):
    guided_multistep(noise_pred, n_branch, g, x_in, x_out, ca, c_cur, s_x, s_e, hist=hist, store_slot=store_slot, hist_idx=hist_idx,
                     w=w, g2=g2)
    _add_noise(x_out, c_noise, seed, stream, step, noise)


class ContractOps:
    """the `ops` a plan launches on: the contracts above (and copy), nothing else"""
    EMULATED = True
    guided_step_sde = staticmethod(guided_step_sde)
    guided_multistep_sde = staticmethod(guided_multistep_sde)
    guided_step = staticmethod(emu_ops.guided_step)
    guided_multistep = staticmethod(guided_multistep)
    copy = staticmethod(emu_ops.copy)


class Bufs:
    """what a plan's `launch` finds on the engine"""

    def __init__(self, x, key):
        self._hist = torch.zeros((4,) + tuple(x.shape), dtype=x.dtype)
        self._saved = torch.empty_like(x)
        self._x_last = torch.zeros_like(x)
        self._noise_key = key


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def alpha_sigma(sig):
    a = 1.0 / math.sqrt(1.0 + sig * sig)
    return a, sig * a


def multistep_moments(s, i, p):
    """(coefficient of the mean, variance) after plan p of step i on point-mass data x0 with eps = (x - alpha_s x0) / sigma_s: every
    data prediction, this step's and the ring's, is x0 itself, so x' = ca x + (c_cur + sum w) x0 + c_noise z"""
    a_s, s_s = alpha_sigma(float(s.sigmas[i]))
    return p.ca * a_s + p.c_cur + sum(p.hist_w), p.ca ** 2 * s_s ** 2 + p.c_noise ** 2


def gaussian_final_variance(s, n, v0=1.0):
    """Data N(0, v0), exact eps = sigma_t x / (alpha_t^2 v0 + sigma_t^2), start x ~ N(0, alpha^2 v0 + sigma^2) at sigmas[0]: every
    data prediction is a multiple of the x it was made from, so the joint law of (x_i, d_{i-1}) stays a centred Gaussian whose
    2 x 2 covariance the plans propagate in closed form.  -> (variance of x after n steps, the exact one at sigmas[n])"""
    s.set_timesteps(n)
    a0, s0 = alpha_sigma(float(s.sigmas[0]))
    cov = np.array([[a0 * a0 * v0 + s0 * s0, 0.0], [0.0, 0.0]])           # state (x, d of the step before)
    for i in range(n):
        p = s.plan_step(i)
        a_s, s_s = alpha_sigma(float(s.sigmas[i]))
        k = s_s / (a_s * a_s * v0 + s_s * s_s)                              # eps = k x
        dx = p.s_x + p.s_e * k                                              # d = dx x
        assert len(p.hist_idx) <= 1
        w = p.hist_w[0] if p.hist_idx else 0.0
        A = np.array([[p.ca + p.c_cur * dx, w], [dx, 0.0]])
        cov = A @ cov @ A.T
        cov[0, 0] += p.c_noise ** 2
    a_n, s_n = alpha_sigma(float(s.sigmas[n]))
    return cov[0, 0], a_n * a_n * v0 + s_n * s_n
