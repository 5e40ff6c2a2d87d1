"""Waveform -> normalised log-mel spectrogram on the device, host side of `avsd_kaldi_fbank`.

Mirrors `waveform_to_melspectrogram` / `AudioMelspectrogramExtractor` of the reference (avgen/data/utils.py:26-110):
centre-crop the waveform to `clip_duration` seconds, ImageBind `waveform2melspec` (un-vendored submodule
facebookresearch/ImageBind, imagebind/data.py: `waveform -= waveform.mean()`, then
`torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=sr, use_energy=False, window_type="hanning",
num_mel_bins, dither=0.0, frame_length=25, frame_shift=10)`, transpose to (mel, time), zero-pad / crop to
`target_length` frames) and `Normalize(mean, std)`.

Neither ImageBind nor torchaudio is in the reference tree or in this image: the filterbank below restates the published
Kaldi algorithm with torchaudio's defaults (povey-free hanning window, pre-emphasis 0.97, per-frame DC removal,
snip_edges, power spectrum, 20 Hz .. Nyquist mel triangles on the 1127 ln(1 + f / 700) scale, log floor at float32
eps) — parity unpinned (oracle/audio_ref.py says the same).  The whole-clip mean subtraction of waveform2melspec is
dropped: the per-frame DC removal that follows cancels any constant offset exactly.

`resample` is the sample-rate converter in front of it, host side of `avsd_resample_sinc_f32`: the reference brings every
real input to 16 kHz with `torchaudio.functional.resample` (avgen/data/utils.py:259,404, compute_avsync.py:141,157).
`resample_taps` restates torchaudio's published windowed-sinc filter bank (`_get_sinc_resample_kernel`) in float64 and is
the only place the filter is defined; torchaudio is not in this image either, so this too is parity unpinned: the filter
is checked against its definition and against closed-form answers (tests/test_resample_cpu.py), not against torchaudio.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def kaldi_mel_banks(num_bins: int = 128, nfft: int = 512, sample_freq: float = 16000.0, low_freq: float = 20.0,
                    high_freq: float = 0.0) -> np.ndarray:
    """[num_bins][nfft/2 + 1] float32 triangular filters (torchaudio `get_mel_banks` + the zero Nyquist column)."""
    nyquist = 0.5 * sample_freq
    if high_freq <= 0.0:
        high_freq += nyquist
    n_fft_bins = nfft // 2
    bin_width = sample_freq / nfft
    mel_low, mel_high = _mel(low_freq), _mel(high_freq)
    delta = (mel_high - mel_low) / (num_bins + 1)
    left = mel_low + np.arange(num_bins, dtype=np.float64)[:, None] * delta
    center, right = left + delta, left + 2.0 * delta
    mel = _mel(bin_width * np.arange(n_fft_bins, dtype=np.float64))[None, :]
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    fb = np.maximum(0.0, np.minimum(up, down))
    return np.concatenate([fb, np.zeros((num_bins, 1))], 1).astype(np.float32)


def hanning_window(n: int) -> np.ndarray:
    """torch.hann_window(n, periodic=False)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1))).astype(np.float32)


class _Tables:
    """Window + filterbank for one (sample_rate, num_mel_bins) pair, uploaded once per device."""

    def __init__(self):
        self._cache = {}

    def get(self, device, sample_rate: int, num_mel_bins: int):
        key = (str(device), sample_rate, num_mel_bins)
        t = self._cache.get(key)
        if t is None:
            win = int(sample_rate * 0.025)
            shift = int(sample_rate * 0.010)
            nfft = 1 << (win - 1).bit_length()                    # round_to_power_of_two
            t = (torch.from_numpy(hanning_window(win)).to(device),
                 torch.from_numpy(kaldi_mel_banks(num_mel_bins, nfft, float(sample_rate))).to(device), shift, nfft)
            self._cache[key] = t
        return t


_TABLES = _Tables()


# ---- sample-rate conversion ------------------------------------------------------------------------------------------
RESAMPLING_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
KAISER_BETA = 14.769656459379492              # torchaudio's default for sinc_interp_kaiser
MAX_TAPS = 1 << 24                            # floats in a filter bank; avsd_resample_sinc_f32 refuses more


def _int_rate(v, name: str) -> int:
    if isinstance(v, bool) or int(v) != v or int(v) <= 0:
        raise ValueError(f"resample: {name} must be a positive integer sample rate, got {v!r}")
    return int(v)


def _resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method) -> Tuple[int, int, int, float]:
    """-> (orig, new, width, base); every argument error of `resample` / `resample_taps` is raised here, on the host."""
    if resampling_method not in RESAMPLING_METHODS:
        raise ValueError(f"resample: unknown resampling_method {resampling_method!r}; one of {RESAMPLING_METHODS}")
    orig_freq, new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")
    if lowpass_filter_width <= 0 or not rolloff > 0.0:
        raise ValueError("resample: lowpass_filter_width and rolloff must be positive")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * float(rolloff)
    width = int(math.ceil(lowpass_filter_width * orig / base))
    L = 2 * width + orig
    if new * L > MAX_TAPS:
        raise ValueError(f"resample: {orig_freq} -> {new_freq} Hz reduces to {orig} : {new}, a filter bank of {new} x {L} taps "
                         f"(more than {MAX_TAPS} floats); rates with a larger common divisor are needed")
    return orig, new, width, base


def resample_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                  resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None) -> Tuple[np.ndarray, int, int, int]:
    """-> (taps f32 [new][L], width, orig, new): torchaudio's polyphase windowed-sinc filter bank, L = 2 * width + orig, with
    orig : new the two rates divided by their gcd.  Output sample q * new + p is sum_k taps[p][k] * x[q * orig + k - width]
    (x zero outside the clip).  Computed in float64, cast to f32 at the end."""
    orig, new, width, base = _resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method)
    k = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    p = np.arange(new, dtype=np.float64)[:, None] / new
    t = np.clip((k - p) * base, -lowpass_filter_width, lowpass_filter_width)
    if resampling_method == "sinc_interp_hann":
        window = np.cos(t * math.pi / lowpass_filter_width / 2.0) ** 2
    else:
        b = KAISER_BETA if beta is None else float(beta)
        window = np.i0(b * np.sqrt(np.maximum(1.0 - (t / lowpass_filter_width) ** 2, 0.0))) / np.i0(b)
    t = t * math.pi
    sinc = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t))
    taps = sinc * window * (base / orig)
    return np.ascontiguousarray(taps.astype(np.float32)), width, orig, new


def resample_length(n_samples: int, orig_freq: int, new_freq: int) -> int:
    """samples `resample` returns for n_samples: ceil(new_freq * n_samples / orig_freq), in integers"""
    orig_freq, new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")
    g = math.gcd(orig_freq, new_freq)
    return (new_freq // g * int(n_samples) + orig_freq // g - 1) // (orig_freq // g)


class _ResampleTaps:
    """Filter banks uploaded once per (device, rates, filter parameters), as _Tables."""

    def __init__(self):
        self._cache = {}

    def get(self, device, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
        g = math.gcd(int(orig_freq), int(new_freq))
        key = (str(device), int(orig_freq) // g, int(new_freq) // g, lowpass_filter_width, float(rolloff), resampling_method,
               None if beta is None else float(beta))
        t = self._cache.get(key)
        if t is None:
            taps, width, orig, new = resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
            t = (torch.from_numpy(taps).to(device), width, orig, new)
            self._cache[key] = t
        return t


_RESAMPLE_TAPS = _ResampleTaps()


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None, device=None) -> torch.Tensor:
    """`torchaudio.functional.resample` on the device: (..., time) -> (..., ceil(new_freq * time / orig_freq)).  Equal rates
    return `waveform` itself, as torchaudio does.  A host tensor is uploaded to `device` (default: cuda); the result stays on
    the device it was computed on, in the dtype of the input (the arithmetic is f32)."""
    _resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method)
    if int(orig_freq) == int(new_freq):
        return waveform
    if not isinstance(waveform, torch.Tensor) or not waveform.is_floating_point() or waveform.dim() < 1 or waveform.numel() == 0:
        raise ValueError("resample: waveform must be a non-empty floating-point tensor (..., time)")
    if device is None:
        device = waveform.device if waveform.is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"resample: the resampler runs on the GPU only (asked for {device}, "
                           f"torch.cuda.is_available() = {torch.cuda.is_available()}); there is no host path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    taps, width, orig, new = _RESAMPLE_TAPS.get(device, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    lead = waveform.shape[:-1]
    rows = waveform.reshape(-1, waveform.shape[-1]).to(device=device, dtype=torch.float32).contiguous()
    with torch.cuda.device(device):
        out = ops.resample_sinc_f32(rows, taps, orig, new, width)
    return out.view(*lead, out.shape[-1]).to(waveform.dtype)


def waveform_to_melspectrogram(waveform: Union[np.ndarray, torch.Tensor], num_mel_bins: int = 128, target_length: int = 204,
                               sample_rate: int = 16000, clip_duration: float = 2.0, mean: float = -4.268, std: float = 9.138,
                               device=None) -> torch.Tensor:
    """(channels, samples) waveform -> (1, num_mel_bins, target_length) f32 on `device` (default: cuda)."""
    if isinstance(waveform, np.ndarray):
        waveform = torch.from_numpy(waveform)
    if waveform.dim() != 2:
        raise ValueError(f"waveform must be (channels, samples), got {tuple(waveform.shape)}")
    n = waveform.shape[1]
    n_target = int(clip_duration * sample_rate)
    start = (n - n_target) // 2 if n > n_target else 0
    if device is None:
        device = waveform.device if waveform.is_cuda else torch.device("cuda")
    clip = waveform[:1, start:start + n_target].to(device=device, dtype=torch.float32).contiguous()   # kaldi.fbank: channel 0
    window, mel_fb, shift, nfft = _TABLES.get(device, sample_rate, num_mel_bins)
    return ops.kaldi_fbank(clip, window, mel_fb, shift=shift, nfft=nfft, t_out=target_length, mean=mean, std=std)


class AudioMelspectrogramExtractor:
    """Same constructor / call contract as the reference class (avgen/data/utils.py:58-110): list of (c, n) waveforms
    -> (b, 1, num_mel_bins, target_length) features."""

    def __init__(self, num_mel_bins=128, target_length=204, sample_rate=16000, clip_duration=2, mean=-4.268, std=9.138):
        self.num_mel_bins = num_mel_bins
        self.target_length = target_length
        self.sample_rate = sample_rate
        self.clip_duration = clip_duration
        self.mean = mean
        self.std = std

    @property
    def max_length_s(self) -> int:
        return self.clip_duration

    @property
    def sampling_rate(self) -> int:
        return self.sample_rate

    def __call__(self, waveforms: Union[np.ndarray, torch.Tensor, List[np.ndarray], List[torch.Tensor]], device=None) -> torch.Tensor:
        if isinstance(waveforms, (np.ndarray, torch.Tensor)) and waveforms.ndim == 2:
            waveforms = [waveforms]
        feats = [waveform_to_melspectrogram(w, self.num_mel_bins, self.target_length, self.sample_rate, self.clip_duration,
                                            self.mean, self.std, device=device) for w in waveforms]
        return torch.stack(feats, 0)      # (b, 1, n_mel, t)
