"""avsd_resample_sinc_f32 on the MI355X against the float64 reference of tests/resample_ref.py, and its wiring into
audio_features.resample, the loaders of data_utils and the AVSync metric.

Accuracy bound (derived, not measured): the kernel adds L products, each rounded once, in f32; whatever the order,
|out - exact| <= gamma_L * sum_k |tap_k * x_k| with gamma_L = L u / (1 - L u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1).  The reference uses the same f32 taps and samples, so nothing else separates the two."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import avsync_ref as AR
from tests import resample_ref as R
from tests.helpers import ROOT, load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = list(R.RATE_PAIRS)


def _bank(orig_freq, new_freq, method="sinc_interp_hann"):
    from asva_amd.audio_features import resample_taps

    taps, width, orig, new = resample_taps(orig_freq, new_freq, resampling_method=method)
    return taps, torch.from_numpy(taps).to(DEV), width, orig, new


def _lengths(orig_freq, orig):
    from asva_amd import ops

    ns = [1, orig - 1, orig, orig + 1, 7 * orig + 5, 2 * orig_freq]
    for qt in ops.RESAMPLE_QT:                       # the two lengths that straddle a workgroup's tile, for either tile
        ns += [qt * orig - 1, qt * orig + 1]
    return sorted({n for n in ns if n > 0})


def _check_against_reference(x, taps, taps_d, width, orig, new):
    from asva_amd import ops

    out = ops.resample_sinc_f32(x.to(DEV), taps_d, orig, new, width)
    ref = R.resample_ref(x, taps, width, orig, new)
    assert out.shape == ref.shape and out.dtype == torch.float32
    bound = R.gamma(taps.shape[1]) * R.abs_sum_ref(x, taps, width, orig, new) + 1e-30
    err = (out.cpu().double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"  {orig}:{new} n_in={x.shape[-1]:6d} n_out={out.shape[-1]:6d}  max |err| {err.max().item():.3e}  max err/bound {worst:.3f}")
    assert bool((err <= bound).all()), (orig, new, x.shape, worst)
    return out


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_matches_float64_reference(pair):
    taps, taps_d, width, orig, new = _bank(*pair)
    for i, n in enumerate(_lengths(pair[0], orig)):
        _check_against_reference(R.make_signal(n, pair[0], seed=100 + i), taps, taps_d, width, orig, new)


def test_kaiser_window_and_decimation_too_long_for_lds():
    """the other window is only other data; 1000 -> 1 Hz (L = 13,122) is the path that reads the row without staging it"""
    taps, taps_d, width, orig, new = _bank(44100, 16000, "sinc_interp_kaiser")
    _check_against_reference(R.make_signal(7 * orig + 5, 44100, seed=7), taps, taps_d, width, orig, new)
    taps, taps_d, width, orig, new = _bank(1000, 1)
    assert (orig, new, width) == (1000, 1, 6061)
    for i, n in enumerate((1, 999, 1000, 1001, 7005, 64 * 1000 - 1, 64 * 1000 + 1)):
        _check_against_reference(R.make_signal(n, 1000, seed=200 + i), taps, taps_d, width, orig, new)


@pytest.mark.parametrize("pair", [(44100, 16000), (48000, 16000), (8000, 16000), (1000, 1)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_no_access_outside_the_rows(pair):
    """input rows inside a NaN-filled buffer, output rows inside a sentinel-filled one, both with margins in front and behind"""
    from asva_amd import ops

    _t, taps_d, width, orig, new = _bank(*pair)
    n_wav, margin, sentinel = 3, 1000, -777.0
    for n_in in (orig + 1, 64 * orig + 1, 256 * orig - 1):
        n_out = R.out_length(n_in, orig, new)
        xs, os_ = n_in + 13, n_out + 29
        x = R.make_signal(n_in, pair[0], seed=n_in % 1000, channels=n_wav).to(DEV)
        xbuf = torch.full((2 * margin + n_wav * xs,), float("nan"), device=DEV)
        xrows = xbuf[margin:margin + n_wav * xs].view(n_wav, xs)[:, :n_in]
        xrows.copy_(x)
        obuf = torch.full((2 * margin + n_wav * os_,), sentinel, device=DEV)
        orows = obuf[margin:margin + n_wav * os_].view(n_wav, os_)[:, :n_out]
        assert xrows.stride(0) == xs and orows.stride(0) == os_
        got = ops.resample_sinc_f32(xrows, taps_d, orig, new, width, out=orows)
        tight = ops.resample_sinc_f32(x, taps_d, orig, new, width)
        assert got.data_ptr() == orows.data_ptr()
        assert bool(torch.isfinite(got).all()) and torch.equal(got, tight)
        outside = torch.ones_like(obuf, dtype=torch.bool)
        outside[margin:margin + n_wav * os_].view(n_wav, os_)[:, :n_out] = False
        assert bool((obuf[outside] == sentinel).all())
        assert bool(torch.isnan(xbuf).sum() == xbuf.numel() - n_wav * n_in)          # and the input is as it was


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_shift_by_one_period_is_exact(pair):
    """`orig` zeros in front move every output by `new` samples, bit for bit: same taps, same samples, same order"""
    from asva_amd import ops

    taps, taps_d, width, orig, new = _bank(*pair)
    n = 2 * pair[0] + 3
    x = R.make_signal(n, pair[0], seed=11)
    shifted = torch.cat([torch.zeros(2, orig), x], dim=1)
    a = ops.resample_sinc_f32(x.to(DEV), taps_d, orig, new, width)
    b = ops.resample_sinc_f32(shifted.to(DEV), taps_d, orig, new, width)
    assert b.shape[1] == a.shape[1] + new and torch.equal(b[:, new:], a)
    # the first `new` samples: what the filter's last `width` taps pick up from the start of x behind the zeros
    ref = R.resample_ref(shifted, taps, width, orig, new)[:, :new]
    bound = R.gamma(taps.shape[1]) * R.abs_sum_ref(shifted, taps, width, orig, new)[:, :new] + 1e-30
    assert bool(((b[:, :new].cpu().double() - ref).abs() <= bound).all())


def test_rows_do_not_depend_on_the_batch_or_the_build():
    from asva_amd import ops, precision

    outs = {}
    for build in ("bf16", "fp16"):
        precision.set_precision(build)
        try:
            for pair in ((44100, 16000), (48000, 16000), (8000, 16000)):
                _t, taps_d, width, orig, new = _bank(*pair)
                x = R.make_signal(70 * orig + 3, pair[0], seed=5, channels=8).to(DEV)
                full = ops.resample_sinc_f32(x, taps_d, orig, new, width)
                for i in range(8):
                    assert torch.equal(full[i:i + 1], ops.resample_sinc_f32(x[i:i + 1], taps_d, orig, new, width)), (build, pair, i)
                outs[build, pair] = full.clone()
        finally:
            precision.set_precision("bf16")
    for (build, pair), v in outs.items():
        assert torch.equal(v, outs["bf16", pair]), (build, pair)


def test_ops_refuses_bad_arguments():
    from asva_amd import ops

    _t, taps_d, width, orig, new = _bank(48000, 16000)
    x = torch.zeros(2, 100, device=DEV)
    assert ops.resample_sinc_f32(x, taps_d, orig, new, width).shape == (2, 34)
    for bad_x, bad_taps in ((x.cpu(), taps_d), (x, taps_d.cpu()), (x.double(), taps_d), (x, taps_d.double()), (x, taps_d[:, :-1]),
                            (x, taps_d.t().contiguous()), (x[0], taps_d), (x[:, ::2], taps_d)):
        with pytest.raises(ValueError):
            ops.resample_sinc_f32(bad_x, bad_taps, orig, new, width)
    with pytest.raises(ValueError):
        ops.resample_sinc_f32(x, taps_d, orig, new, width, out=torch.empty(2, 33, device=DEV))


def test_resample_host_and_device_inputs_agree():
    from asva_amd.audio_features import resample, resample_length

    x = R.make_signal(22050, 22050, seed=2, channels=6).view(2, 3, 22050)
    a = resample(x.to(DEV), 22050, 16000)
    b = resample(x, 22050, 16000, device=DEV)
    c = resample(x, 22050, 16000)
    assert a.is_cuda and b.is_cuda and c.is_cuda and a.shape == (2, 3, 16000) == (2, 3, resample_length(22050, 22050, 16000))
    assert torch.equal(a, b) and torch.equal(a, c)
    taps, _d, width, orig, new = _bank(22050, 16000)
    bound = R.gamma(taps.shape[1]) * R.abs_sum_ref(x, taps, width, orig, new) + 1e-30
    assert bool(((a.cpu().double() - R.resample_ref(x, taps, width, orig, new)).abs() <= bound).all())
    k = resample(x[0, 0], 22050, 16000, resampling_method="sinc_interp_kaiser", device=DEV)
    assert k.shape == (16000,) and not torch.equal(k, a[0, 0])
    assert resample(x.double(), 22050, 16000, device=DEV).dtype == torch.float64


def test_loader_resamples_on_the_device(tmp_path):
    from asva_amd import data_utils as D
    from asva_amd.audio_features import resample

    rng = np.random.default_rng(0)
    frames = rng.integers(0, 255, (60, 24, 32, 3), dtype=np.uint8)                  # 2 s at 30 fps
    audio = (rng.standard_normal((2, 44100)) * 0.1).astype(np.float32)               # 2 s at 22.05 kHz
    np.savez(tmp_path / "v.npz", frames=frames, fps=30.0, audio=audio, audio_sr=22050)

    def load():
        return D.load_av_clips_uniformly(str(tmp_path / "v.npz"), video_fps=6, video_num_frame=6, image_size=(24, 32), num_clips=2,
                                         load_audio_as_melspectrogram=False)

    vid_h, aud_h = load()
    D.set_resampler("device")
    try:
        assert D.get_resampler() == "device"
        vid_d, aud_d = load()
    finally:
        D.set_resampler("host")
    assert torch.equal(vid_d, vid_h) and len(aud_d) == len(aud_h) == 2
    for t0, got, host in zip((0.0, 1.0), aud_d, aud_h):
        assert not got.is_cuda and got.dtype == torch.float32 and got.shape == host.shape == (2, 16000)
        piece = torch.from_numpy(audio[:, int(round(t0 * 22050)):int(round((t0 + 1.0) * 22050))])
        assert torch.equal(got, resample(piece, 22050, 16000).cpu())
        assert not torch.equal(got, host)                                          # the host filter is another filter


@pytest.fixture(scope="module")
def net():
    from asva_amd import avsync as A

    g = load_golden("avsync_tiny.pt")
    sd = AR.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    m = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    m.load_state_dict(sd)
    return m.to(DEV)


def test_sync_metric_resamples_on_the_device(net):
    from asva_amd import avsync as A
    from asva_amd import data_utils as D
    from asva_amd.audio_features import resample

    t = torch.arange(88200, dtype=torch.float32) / 44100.0
    wave = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) * (1.0 + torch.sin(2 * torch.pi * 3.0 * t)))[None]
    wave2 = (0.2 * torch.sin(2 * torch.pi * 1200.0 * t[::2] * (1.0 + 0.2 * t[::2])))[None]            # 2 s at 22.05 kHz
    clip = AR.u8_to_unit(AR.grating_video_u8(12, 256, 256, 0.7, 0.13, 23.0))
    D.set_resampler("device")
    try:
        score = A.compute_sync_metrics_on_av(wave, 44100, clip, metric="avsync_score", net=net)
        rel = A.compute_sync_metrics_on_av(wave, 44100, clip, ref_audio_waveform=wave2, ref_audio_sr=22050, metric="relsync", net=net)
    finally:
        D.set_resampler("host")
    w16, w16b = resample(wave, 44100, 16000, device=DEV), resample(wave2, 22050, 16000, device=DEV)
    assert w16.shape == (1, 32000)
    assert torch.equal(score, A.compute_sync_metrics_on_av(w16, 16000, clip, metric="avsync_score", net=net))
    assert torch.equal(rel, A.compute_sync_metrics_on_av(w16, 16000, clip, ref_audio_waveform=w16b, metric="relsync", net=net))
    assert bool(torch.isfinite(score)) and 0.0 < float(rel) < 1.0
    with pytest.raises(ValueError, match="16000"):                                  # back on "host": as before
        A.compute_sync_metrics_on_av(wave, 44100, clip, metric="avsync_score", net=net)


def test_resample_bench_tool_runs():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "resample_bench.py"), "--quick"],
                       capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "log-mel" in r.stdout and "44100" in r.stdout
