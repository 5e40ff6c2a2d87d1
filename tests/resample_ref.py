"""Float64 reference of the sample-rate converter (asva_amd/audio_features.py:resample, avsd_resample_sinc_f32), written the way
torchaudio applies its filter bank: zero-pad the waveform by (width, width + orig), one strided conv1d with the `new` filter
rows as output channels, interleave the channels (phases) in time, cut to ceil(new * n / orig).  The taps are the f32 ones of
`resample_taps`, widened: the reference and the kernel differ by the kernel's summation error only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (orig_freq, new_freq) -> (orig, new, width, L): the conversions the tests run, with the known filter geometry
RATE_PAIRS = {
    (48000, 16000): (3, 1, 19, 41),
    (44100, 16000): (441, 160, 17, 475),
    (22050, 16000): (441, 320, 9, 459),
    (8000, 16000): (1, 2, 7, 15),
    (32000, 16000): (2, 1, 13, 28),
    (11025, 16000): (441, 640, 7, 455),
}


def out_length(n: int, orig: int, new: int) -> int:
    return (new * n + orig - 1) // orig


def _apply(x: torch.Tensor, taps: torch.Tensor, width: int, orig: int, new: int) -> torch.Tensor:
    lead, n = x.shape[:-1], x.shape[-1]
    xp = F.pad(x.reshape(-1, 1, n), (width, width + orig))
    y = F.conv1d(xp, taps[:, None, :], stride=orig)                 # (rows, new, n // orig + 1)
    y = y.transpose(1, 2).reshape(y.shape[0], -1)[:, :out_length(n, orig, new)]
    return y.reshape(*lead, y.shape[-1])


def resample_ref(x, taps, width: int, orig: int, new: int) -> torch.Tensor:
    """x (..., n), taps f32 [new][2 * width + orig] -> float64 (..., ceil(new * n / orig))"""
    x = torch.as_tensor(np.asarray(x)).double()
    taps = torch.as_tensor(np.asarray(taps)).double()
    assert tuple(taps.shape) == (new, 2 * width + orig)
    return _apply(x, taps, width, orig, new)


def abs_sum_ref(x, taps, width: int, orig: int, new: int) -> torch.Tensor:
    """sum_k |tap_k * x_k| per output sample, float64: the scale of the rounding-error bound"""
    x = torch.as_tensor(np.asarray(x)).double().abs()
    taps = torch.as_tensor(np.asarray(taps)).double().abs()
    return _apply(x, taps, width, orig, new)


def gamma(L: int) -> float:
    """worst-case relative error of any f32 summation of L products, each rounded once (Higham, gamma_n with u = 2^-24)"""
    u = L * 2.0 ** -24
    return u / (1.0 - u)


def make_signal(n: int, rate: int, seed: int, channels: int = 2) -> torch.Tensor:
    """seeded noise plus a sine, f32 (channels, n)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / rate
    rows = [0.1 * torch.randn(n, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2 * math.pi * (440.0 + 170.0 * c) * t + c)
            for c in range(channels)]
    return torch.stack(rows).float()
