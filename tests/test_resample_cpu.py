"""Sample-rate conversion, the parts that need no GPU: the filter bank of asva_amd/audio_features.py:resample_taps against its
known geometry and closed-form answers (torchaudio itself is absent: parity unpinned), the float64 reference of
tests/resample_ref.py, output lengths, the host/device switch of asva_amd/data_utils.py and the argument checks of
avsd_resample_sinc_f32."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as R

METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")


@pytest.fixture(scope="module")
def banks():
    """(orig_freq, new_freq, method) -> (taps, width, orig, new), built once"""
    from asva_amd.audio_features import resample_taps

    return {(o, n, m): resample_taps(o, n, resampling_method=m) for (o, n) in R.RATE_PAIRS for m in METHODS}


def test_filter_geometry_known_values(banks):
    for (o, n, m), (taps, width, orig, new) in banks.items():
        assert (orig, new, width, taps.shape[1]) == R.RATE_PAIRS[(o, n)], (o, n, m)
        assert taps.dtype == np.float32 and taps.shape == (new, 2 * width + orig) and taps.flags["C_CONTIGUOUS"]
    # the definition, spelled out for one tap: 44.1 -> 16 kHz, phase 7, tap 40
    taps, width, orig, new = banks[(44100, 16000, "sinc_interp_hann")]
    base = 160 * 0.99
    t = ((40 - width) / orig - 7 / new) * base
    want = math.sin(math.pi * t) / (math.pi * t) * math.cos(math.pi * t / 12.0) ** 2 * base / orig
    assert abs(t) < 6 and abs(float(taps[7, 40]) - want) <= 2e-7 * abs(want)          # f32 rounding of the float64 value
    # outside +-lowpass_filter_width zero crossings the window (hann) is zero
    assert abs(float(taps[0, -1])) < 1e-12 and abs(float(taps[new - 1, 0])) < 1e-12
    # a filter-width and a rolloff other than the defaults move the width as the definition says
    from asva_amd.audio_features import resample_taps

    assert resample_taps(48000, 16000, lowpass_filter_width=16, rolloff=0.9475937167399596)[1] == 51
    b12 = resample_taps(8000, 16000, resampling_method="sinc_interp_kaiser", beta=12.0)[0]
    assert not np.array_equal(b12, banks[(8000, 16000, "sinc_interp_kaiser")][0])


def test_dc_gain_of_every_phase(banks):
    """a wrong base / orig scale or a wrong window is an error of a factor; measured: at most 8.75e-4 (hann), 2.5e-7 (kaiser)"""
    for (o, n, m), (taps, *_r) in banks.items():
        dev = np.abs(taps.astype(np.float64).sum(axis=1) - 1.0).max()
        assert dev < (2e-3 if m == "sinc_interp_hann" else 1e-6), (o, n, m, dev)


def test_sine_through_the_reference(banks):
    """1 kHz, 2 s: the resampled sine is the sine at the new rate; measured: at most 1.0e-3 (hann), 4.0e-6 (kaiser)"""
    for (o, n, m), (taps, width, orig, new) in banks.items():
        x = torch.sin(2 * math.pi * 1000.0 * torch.arange(2 * o, dtype=torch.float64) / o)
        y = R.resample_ref(x, taps, width, orig, new)
        assert y.shape == (2 * n,)
        want = torch.sin(2 * math.pi * 1000.0 * torch.arange(2 * n, dtype=torch.float64) / n)
        err = (y - want)[200:-200].abs().max().item()
        assert err < (2e-3 if m == "sinc_interp_hann" else 1e-5), (o, n, m, err)


LENGTHS = [(44100, 1, 1), (44100, 2, 1), (44100, 3, 2), (44100, 440, 160), (44100, 441, 160), (44100, 442, 161),
           (48000, 440, 147), (48000, 441, 147), (48000, 442, 148), (8000, 3, 6)]


def test_output_lengths(banks):
    from asva_amd import _lib
    from asva_amd.audio_features import resample_length

    h = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before a launch
    for o, T, want in LENGTHS:
        taps, width, orig, new = banks[(o, 16000, "sinc_interp_hann")]
        assert resample_length(T, o, 16000) == want
        assert R.resample_ref(torch.zeros(2, T), taps, width, orig, new).shape == (2, want)
        # the library computes the same length, in integers: one more or one less is refused, and the message names `want`
        for bad in (want - 1, want + 1):
            if bad <= 0:
                continue
            assert h.avsd_resample_sinc_f32(fake, 1, T, T, fake, orig, new, width, fake, bad, bad, None) == -1
            assert re.search(rb"= (\d+)$", h.avsd_last_error()).group(1) == str(want).encode()
    assert resample_length(2 ** 31 - 1, 44100, 16000) == (160 * (2 ** 31 - 1) + 440) // 441      # no 32-bit overflow


def test_entry_point_reports_argument_errors_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    p = ctypes.c_void_p(4096)
    orig, new, width, n_in, n_out = 441, 160, 17, 1000, 363
    good = dict(x=p, n_wav=2, n_in=n_in, x_stride=n_in, taps=p, orig=orig, new=new, width=width, out=p, n_out=n_out, out_stride=n_out)

    def call(**kw):
        a = dict(good, **kw)
        rc = h.avsd_resample_sinc_f32(a["x"], a["n_wav"], a["n_in"], a["x_stride"], a["taps"], a["orig"], a["new"], a["width"], a["out"],
                                      a["n_out"], a["out_stride"], None)
        return rc, h.avsd_last_error()

    for name in ("x", "taps", "out"):
        rc, msg = call(**{name: None})
        assert rc == -1 and b"null pointer" in msg, name
    for name in ("n_wav", "n_in", "orig", "new", "width", "n_out"):
        for v in (0, -3):
            rc, msg = call(**{name: v})
            assert rc == -1 and b"bad sizes" in msg, (name, v)
    rc, msg = call(n_out=n_out + 1, out_stride=n_out + 1)
    assert rc == -1 and b"n_out" in msg and b"363" in msg
    rc, msg = call(x_stride=n_in - 1)
    assert rc == -1 and b"strides" in msg
    rc, msg = call(out_stride=n_out - 1)
    assert rc == -1 and b"strides" in msg
    # 44101 -> 16000 Hz is co-prime: 16000 x 44135 taps
    rc, msg = call(orig=44101, new=16000, width=17, n_in=44101, x_stride=44101, n_out=16000, out_stride=16000)
    assert rc == -1 and b"2^24" in msg
    rc, msg = call(orig=1, new=1 << 23, width=1, n_in=1, x_stride=1, n_out=1 << 23, out_stride=1 << 23)      # 3 * 2^23 floats
    assert rc == -1 and b"2^24" in msg


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from asva_amd import _lib, ops
    from asva_amd.audio_features import resample, resample_taps

    def no_lib():
        raise AssertionError("the kernel library was asked for")

    monkeypatch.setattr(_lib, "lib", no_lib)
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="sinc_interp_nope"):
        resample(x, 44100, 16000, resampling_method="sinc_interp_nope")
    with pytest.raises(ValueError, match="sinc_interp_nope"):
        resample_taps(44100, 16000, resampling_method="sinc_interp_nope")
    with pytest.raises(ValueError, match="44101"):
        resample(x, 44101, 16000)
    with pytest.raises(ValueError, match="44101"):
        resample_taps(44101, 16000)
    with pytest.raises(ValueError):
        resample(x, 0, 16000)
    with pytest.raises(ValueError):
        resample(x, 44100.5, 16000)
    with pytest.raises(ValueError, match="device tensor"):
        ops.resample_sinc_f32(x, torch.zeros(160, 475), 441, 160, 17)


def test_equal_rates_return_the_input_object():
    from asva_amd.audio_features import resample
    from asva_amd.data_utils import _resample

    x = torch.randn(2, 3, 50)
    assert resample(x, 16000, 16000) is x and resample(x, 44100, 44100, resampling_method="sinc_interp_kaiser") is x
    row = x[0]
    assert _resample(row, 16000, 16000) is row


def test_switch_defaults_to_host_and_host_is_the_old_path(monkeypatch):
    from asva_amd import data_utils as D

    assert D.get_resampler() == "host"
    with pytest.raises(ValueError, match="nowhere"):
        D.set_resampler("nowhere")
    audio = R.make_signal(5000, 22050, seed=3)
    got = D._resample(audio, 22050, 16000)
    try:
        import torchaudio  # type: ignore

        want = torchaudio.functional.resample(audio, orig_freq=22050, new_freq=16000)
    except ImportError:
        from scipy.signal import resample_poly

        want = torch.from_numpy(resample_poly(audio.numpy().astype(np.float64), 320, 441, axis=1).astype(np.float32))
    assert got.dtype == torch.float32 and not got.is_cuda and torch.equal(got, want)
    # "device" without a GPU is refused, and the switch stays where it was
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    try:
        with pytest.raises(RuntimeError, match="no GPU"):
            D.set_resampler("device")
        assert D.get_resampler() == "host"
        from asva_amd.audio_features import resample

        with pytest.raises(RuntimeError, match="GPU only"):
            resample(audio, 22050, 16000)
    finally:
        D.set_resampler("host")


def test_sync_metrics_error_names_the_switch():
    from asva_amd import avsync as A

    wave, clip = torch.zeros(1, 44100), torch.zeros(3, 12, 8, 8)
    with pytest.raises(ValueError, match="16000") as e:
        A.compute_sync_metrics_on_av(wave, 44100, clip, metric="avsync_score")
    assert "set_resampler" in str(e.value) and "44100" in str(e.value)
    with pytest.raises(ValueError, match="set_resampler"):
        A.compute_sync_metrics_on_av(torch.zeros(1, 32000), 16000, clip, ref_audio_waveform=wave, ref_audio_sr=44100, metric="relsync")
