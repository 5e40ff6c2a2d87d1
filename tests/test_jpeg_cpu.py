"""The host side of the on-device JPEG encoder (asva_amd/video_io.py) and the float64 reference the GPU tests compare against
(tests/jpeg_ref.py), checked against libjpeg through PIL: no kernel runs here.

The bound between PIL's decoded pixels and the reference's exact float64 reconstruction of the same coefficients is
libjpeg's integer IDCT and colour rounding.  It is measured by `measure_libjpeg_bound()` below on the in-gamut inputs at
quality 95 and stored, plus 0.5 level, in tests/golden/jpeg/meta.json; the tests assert against the stored value."""
import io
import json
import os
import struct
import warnings

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R
from tests.helpers import ROOT

META = os.path.join(ROOT, "tests", "golden", "jpeg", "meta.json")


def _meta():
    with open(META) as f:
        return json.load(f)


def _decode(data):
    from PIL import Image

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def _pil_encode(frame, quality, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def _bound_inputs():
    named = R.named_frames()
    return [named[n] for n in ("mcu", "noise", "smooth", "flat", "checker")] + list(R.clip_frames())


def measure_libjpeg_bound(quality=95):
    """max |PIL's decode - float64 reconstruction| over the shared inputs: what meta.json's "measured_max_levels" records"""
    qy, qc = R.tables(quality)
    worst = 0.0
    for f in _bound_inputs():
        coef = R.quantize(f, qy, qc)
        dec = np.asarray(_decode(R.jpeg_from_coefficients(coef, f.shape[0], f.shape[1], qy, qc)), dtype=np.float64)
        worst = max(worst, float(np.abs(dec - R.reconstruct(coef, qy, qc)).max()))
    return worst


@pytest.mark.parametrize("quality", [50, 75, 95, 100])
def test_tables_are_the_ones_pil_reports(quality):
    from asva_amd.video_io import jpeg_tables

    qy, qc = jpeg_tables(quality)
    pil = _decode(_pil_encode(R.smooth_image(), quality)).quantization
    assert list(pil[0]) == qy and list(pil[1]) == qc                      # PIL reports natural order
    ry, rc = R.tables(quality)
    assert list(ry) == qy and list(rc) == qc
    for bad in (0, 101):
        with pytest.raises(ValueError):
            jpeg_tables(bad)


def test_header_is_the_reference_header_and_in_marker_order():
    from asva_amd import video_io as V

    qy, qc = V.jpeg_tables(95)
    head = V._jpeg_header(48, 64, qy, qc)
    assert head == R.headers(48, 64, *R.tables(95))
    markers, p = [], 2
    while p < len(head):
        assert head[p] == 0xFF
        markers.append(head[p + 1])
        p += 2 + struct.unpack(">H", head[p + 2:p + 4])[0]
    assert head[:2] == b"\xff\xd8" and markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA] and p == len(head)
    # the DQT segments carry zigzag order: PIL reads back the natural-order tables
    dec = _decode(R.jpeg_from_coefficients(np.zeros((6, 8, 3, 64), dtype=np.int16), 48, 64, qy, qc))
    assert list(dec.quantization[0]) == qy and list(dec.quantization[1]) == qc


@pytest.mark.parametrize("quality", [100, 95, 75])
def test_reference_streams_decode_in_pil(quality):
    qy, qc = R.tables(quality)
    for name, f in R.named_frames().items():
        im = _decode(R.encode(f, quality))
        assert im.size == (f.shape[1], f.shape[0]) and im.mode == "RGB", name
    for name, c in R.handmade_coefficients().items():
        im = _decode(R.jpeg_from_coefficients(c, c.shape[0] * 8, c.shape[1] * 8, qy, qc))
        assert im.size == (c.shape[1] * 8, c.shape[0] * 8) and im.mode == "RGB", name


def test_pil_decode_is_within_the_stored_bound_of_the_float64_reconstruction():
    meta = _meta()
    worst = measure_libjpeg_bound(meta["quality"])
    print(f"max |PIL decode - float64 reconstruction| at quality {meta['quality']}: {worst:.3f} levels (stored bound {meta['libjpeg_bound_levels']})")
    assert meta["libjpeg_bound_levels"] == pytest.approx(meta["measured_max_levels"] + 0.5)
    assert worst <= meta["libjpeg_bound_levels"]


def test_reference_psnr_is_pils_at_equal_tables():
    """quality 95 (the writer's), 4:4:4 on both sides: within 0.1 dB.  Quality 100 and the noise frames at 75 are left out of
    this comparison: at a table of ones libjpeg's integer forward DCT costs it 0.2 - 0.5 dB against any exact encoder, and
    noise at coarse tables leaves the gamut, where the decoder's clipping, not the encoder, decides the figure."""
    named = R.named_frames()
    for name in ("mcu", "noise", "smooth", "flat", "checker"):
        f = named[name]
        ours = R.psnr(np.asarray(_decode(R.encode(f, 95))), f)
        pil = R.psnr(np.asarray(_decode(_pil_encode(f, 95, subsampling=0))), f)
        print(f"{name}: reference {ours:.3f} dB, PIL {pil:.3f} dB")
        assert ours == pil or abs(ours - pil) <= 0.1, (name, ours, pil)


def test_tie_window_cap_holds_for_the_quantiser_inputs():
    """at most 2 % of the quotients of each GPU quantiser case sit within the tie window (the cap the GPU test relies on)"""
    named = R.named_frames()
    for name, q in R.quantize_cases():
        frac = float(R.near_tie(R.quotients(named[name], *R.tables(q))).mean())
        print(f"{name} q{q}: {100 * frac:.2f} % of the quotients within {R.TIE_WINDOW} of a tie")
        assert frac <= 0.02, (name, q, frac)


def test_pack_inputs_cover_stuffing_and_all_bit_residues():
    scans = [R.encode_scan(c) for c in R.handmade_coefficients().values()]
    assert any(b"\xff" in s for s, _ in scans)
    residues = {n % 8 for _, n in scans} | {n % 8 for _, n in (R.encode_scan(c) for c in R.residue_sweep())}
    assert residues == set(range(8))


def test_encoder_setting_and_environment_variable(monkeypatch):
    from asva_amd import video_io as V

    assert V.get_jpeg_encoder() == "host"                                  # the default
    with pytest.raises(ValueError, match="unknown mode"):
        V.set_jpeg_encoder("gpu")
    with pytest.raises(ValueError, match="unknown mode"):
        V._encoder_from_env({"AVSD_JPEG_ENCODER": "gpu"})
    V._encoder_from_env({})
    V._encoder_from_env({"AVSD_JPEG_ENCODER": "host"})
    assert V.get_jpeg_encoder() == "host"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)           # as on a machine without a GPU
    frames = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.set_jpeg_encoder("device")
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V._encoder_from_env({"AVSD_JPEG_ENCODER": "device"})
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.encode_jpeg_frames(frames)
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.write_mjpeg_avi("unused.avi", frames, 6, encoder="device")
    assert V.get_jpeg_encoder() == "host"
    with pytest.raises(ValueError, match="unknown encoder"):
        V.write_mjpeg_avi("unused.avi", np.zeros((1, 8, 8, 3), dtype=np.uint8), 6, encoder="gpu")


def test_default_writer_still_stores_pils_frames(tmp_path):
    """with the default encoder the file is, byte for byte, the container around PIL's own encodes (4:2:0, optimise off)"""
    from asva_amd import video_io as V

    rng = np.random.default_rng(4)
    video = np.stack([R.smooth_image(seed=s) for s in (1, 2, 3)])
    audio = (rng.standard_normal((2, 8000)) * 0.1).astype(np.float32)
    path = V.write_mjpeg_avi(str(tmp_path / "a.avi"), torch.from_numpy(video), 6, torch.from_numpy(audio), 16000)
    data = open(path, "rb").read()
    frames, p = [], data.index(b"movi") + 4
    while data[p:p + 4] == b"00dc":
        n = struct.unpack("<I", data[p + 4:p + 8])[0]
        frames.append(data[p + 8:p + 8 + n])
        p += 8 + n + (n & 1)
    assert frames == [_pil_encode(video[t], 95) for t in range(3)]
    same = V.write_mjpeg_avi(str(tmp_path / "b.avi"), video, 6, audio, 16000, encoder="host")
    assert open(same, "rb").read() == data
    back, fps, aud, afps = V.read_mjpeg_avi(path)
    assert back.shape == (3, 48, 64, 3) and fps == 6.0 and aud.shape == (2, 8000) and afps == 16000
    with pytest.raises(ValueError, match="uint8"):
        V.write_mjpeg_avi(str(tmp_path / "c.avi"), video.astype(np.float32), 6)


def test_generate_videos_asks_for_device_frames_only_when_writing_with_the_device_encoder(monkeypatch, tmp_path):
    from asva_amd import pipeline as P
    from asva_amd import video_io as V

    asked = []

    class Pipe:
        vae_scale_factor = 8

        def __call__(self, **kw):
            asked.append(kw["output_type"])
            return torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)

    clips = [dict(image_latents=torch.zeros(4, 1, 1), audio_encodings=torch.zeros(1, 1), null_audio_encodings=torch.zeros(1, 1))]
    kw = dict(clips=clips, device=torch.device("cpu"), image_size=(8, 8), video_num_frame=2)
    written = []
    P.generate_videos(Pipe(), **kw)
    P.generate_videos(Pipe(), **kw, save_template=str(tmp_path / "y"), writer=lambda *a: written.append(a))
    monkeypatch.setattr(V, "_jpeg_encoder", "device")
    P.generate_videos(Pipe(), **kw)
    P.generate_videos(Pipe(), **kw, save_template=str(tmp_path / "y"), writer=lambda *a: written.append(a))
    assert asked == ["uint8", "uint8", "uint8", "uint8_device"] and len(written) == 2
