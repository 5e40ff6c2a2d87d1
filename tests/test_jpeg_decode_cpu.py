"""The host side of the JPEG decoder and the .avi clip source, without a GPU.

tests/jpeg_dec_ref.py (a Python-integer restatement of libjpeg's default decompression path) must return the bytes PIL returns;
the package's marker parser and Huffman decode tables (asva_amd/video_io.py) must agree with it; `.avi` files must open as clip
sources in the loaders and the evaluation driver."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_dec_ref as D
from tests import jpeg_ref as R


def _pil_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _pil_encode(img, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _image(H, W, seed=5):
    """the smooth test image with +-20 levels of noise: AC energy in every block, in gamut"""
    rng = np.random.default_rng(seed)
    base = R.smooth_image(max(H, 8), max(W, 8))[:H, :W].astype(np.int64)
    return np.clip(base + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)


def _with_dri(data, interval):
    """the stream with a DRI segment in front of its SOS"""
    at = data.index(b"\xff\xda")
    return data[:at] + b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big") + data[at:]


@pytest.mark.parametrize("quality", (50, 95))
def test_restatement_equals_pil_on_444_streams_of_the_encoder_reference(quality):
    data = R.encode(R.smooth_image(48, 64), quality)
    assert np.array_equal(D.decode(data), _pil_decode(data))


@pytest.mark.parametrize("quality", (50, 95, 100))
def test_restatement_equals_pil_on_handmade_coefficients(quality):
    """ZRL runs, coefficient 63, no EOB, the largest categories: the extreme values leave the 16-bit range of libjpeg-turbo's vector
    IDCT, whose wrapping and saturation the restatement (and the kernel) therefore state"""
    qy, qc = R.tables(quality)
    for name, coef in R.handmade_coefficients().items():
        data = R.jpeg_from_coefficients(coef, coef.shape[0] * 8, coef.shape[1] * 8, qy, qc)
        info = D.parse(data)
        assert np.array_equal(D.decode_scan(info).reshape(coef.shape), coef), name
        assert np.array_equal(D.pixels(info, D.decode_scan(info)), _pil_decode(data)), name


@pytest.mark.parametrize("size", ((48, 64), (40, 56), (37, 51), (8, 8)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("quality", (50, 95, 100))
def test_restatement_equals_pil_on_pil_streams(size, quality):
    img = _image(*size)
    for kw in ({}, {"subsampling": 0}, {"optimize": True}):
        data = _pil_encode(img, quality=quality, **kw)
        info = D.parse(data)
        assert info["sampling"] == ("444" if kw.get("subsampling") == 0 else "420") and (info["H"], info["W"]) == size
        assert np.array_equal(D.decode(data), _pil_decode(data)), kw


def _lookup(table, bits16):
    """the kernel's table lookup (include/avsd.h, AVSD_JPEG_HUFF_WORDS) on a 16-bit left-aligned prefix -> (symbol, length) or None"""
    e = int(table[bits16 >> 8])
    if e:
        return e & 0xFF, e >> 8
    for length in range(9, 17):
        if bits16 < int(table[256 + length - 1]):
            idx = ((bits16 >> (16 - length)) + int(table[272 + length - 1])) & 0xFF
            return (int(table[288 + (idx >> 2)]) >> ((idx & 3) * 8)) & 0xFF, length
    return None


def test_parser_and_decode_tables_agree_with_the_restatement():
    from asva_amd import video_io as V

    img = _image(40, 56)
    streams = [R.encode(R.smooth_image(48, 64), 95), _pil_encode(img, quality=75), _pil_encode(img, quality=95, optimize=True),
               _pil_encode(img, quality=50, subsampling=0)]
    for data in streams:
        got, ref = V.parse_jpeg(data), D.parse(data)
        assert (got["H"], got["W"], got["sampling"]) == (ref["H"], ref["W"], ref["sampling"])
        assert [list(q) for q in got["qtabs"]] == ref["qtabs"]
        assert got["scan"].replace(b"\xff\x00", b"\xff") == ref["scan"]
        for c in range(3):
            for which, spec in zip(got["huff"][c], (ref["dc"][c], ref["ac"][c])):
                assert (list(which[0]), list(which[1])) == (list(spec[0]), list(spec[1]))
                table = V.huffman_decode_table(*which, dc=spec is ref["dc"][c])
                assert table.shape == (352,) and table.dtype == np.uint32
                codes = D._decode_table(spec)
                for (length, code), sym in codes.items():                 # every code, followed by zeros and by ones
                    for tail in (0, (1 << (16 - length)) - 1):
                        assert _lookup(table, (code << (16 - length)) | tail) == (sym, length)
                if not any(code == (1 << length) - 1 for (length, code) in codes):
                    assert _lookup(table, 0xFFFF) is None                 # the all-ones prefix belongs to no code


def test_parser_refuses_what_the_device_decoder_does_not_take():
    from PIL import Image

    from asva_amd import video_io as V

    img = _image(40, 56)
    buf = io.BytesIO()
    Image.fromarray(img).convert("L").save(buf, format="JPEG")
    good = _pil_encode(img, quality=90)
    cases = {"progressive": (_pil_encode(img, progressive=True), "progressive"), "greyscale": (buf.getvalue(), "1 component"),
             "4:2:2": (_pil_encode(img, subsampling=1), "sampling factors 2x1"), "restart interval": (_with_dri(good, 4), "restart interval"),
             "no SOI": (good[2:], "SOI"), "cut in the tables": (good[:100], "SOS|cut short")}
    for name, (data, what) in cases.items():
        with pytest.raises(ValueError, match=what):
            V.parse_jpeg(data)
        if name in ("progressive", "greyscale", "4:2:2", "restart interval"):
            with pytest.raises(D.Unsupported):
                D.parse(data)
    V.parse_jpeg(_with_dri(good, 0))                                          # DRI of 0 switches restarts off
    with pytest.raises(ValueError, match="missing"):
        V.parse_jpeg(good.replace(b"\xff\xc4", b"\xff\xe5"))                   # the DHT segments relabelled as APP5: no table
    with pytest.raises(ValueError, match="more codes"):
        V.huffman_decode_table(bytes([3] + [0] * 15), bytes(3), dc=True)
    with pytest.raises(ValueError, match="category"):
        V.huffman_decode_table(bytes([1] + [0] * 15), bytes([12]), dc=True)


def _id_clip():
    """60 frames of 48 x 64 at 30 fps whose 16 x 16 top-left block holds 4 x the frame id (JPEG keeps a flat block within a level or
    two), and 2 s of audio"""
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 255, (60, 48, 64, 3), dtype=np.uint8)
    frames[:, :16, :16] = (4 * np.arange(60, dtype=np.uint8))[:, None, None, None]
    audio = (rng.standard_normal((1, 32000)) * 0.1).astype(np.float32)
    return frames, audio


def test_avi_is_a_clip_source_for_the_loaders(tmp_path):
    """fails before the .avi routing: load_av_clips_uniformly("x.avi") raised RuntimeError("... needs torchvision ...")"""
    from asva_amd import video_io as V
    from asva_amd.data_utils import _MjpegClip, _open_video, load_av_clips_uniformly, load_video_clips_uniformly

    frames, audio = _id_clip()
    path = V.write_mjpeg_avi(str(tmp_path / "v.avi"), frames, 30.0, audio, 16000)
    src = _open_video(path)
    assert isinstance(src, _MjpegClip) and src.fps == 30.0 and src.video_duration == 2.0 and src.audio_duration == 2.0 and src.audio_sr == 16000
    vid, aud = load_av_clips_uniformly(path, video_fps=6, video_num_frame=6, image_size=(48, 64), num_clips=2, load_audio_as_melspectrogram=False)
    assert vid.shape == (2, 6, 3, 48, 64) and not vid.is_cuda and len(aud) == 2 and aud[0].shape == (1, 16000)
    ids = ((vid[0, :, :, 4, 4] * 255).mean(dim=1) / 4).round().int().tolist()
    assert ids == [0, 5, 10, 15, 20, 25]                                       # the frames the .npz test of test_host_cpu.py picks
    # the same clips as the .npz container of the PIL-decoded frames and the stored audio gives
    decoded, fps, stored_audio, afps = V.read_mjpeg_avi(path)
    np.savez(tmp_path / "v.npz", frames=decoded.numpy(), fps=fps, audio=stored_audio.numpy(), audio_sr=afps)
    vid_z, aud_z = load_av_clips_uniformly(str(tmp_path / "v.npz"), video_fps=6, video_num_frame=6, image_size=(48, 64), num_clips=2,
                                           load_audio_as_melspectrogram=False)
    assert torch.equal(vid, vid_z) and all(torch.equal(a, b) for a, b in zip(aud, aud_z))
    assert torch.equal(load_video_clips_uniformly(path, 6, 6, (48, 64), 1), load_video_clips_uniformly(str(tmp_path / "v.npz"), 6, 6, (48, 64), 1))
    # a clip that runs past the end repeats its last frame, as the container does
    assert torch.equal(src.video_clip(1.5, 1.0, 6, 6), _open_video(str(tmp_path / "v.npz")).video_clip(1.5, 1.0, 6, 6))
    # other extensions are routed as before
    (tmp_path / "w.avi").write_bytes(b"RIFF\0\0\0\0WAVEfmt ")
    for other in ("v.mp4", "w.avi"):
        with pytest.raises(RuntimeError, match="torchvision"):
            load_av_clips_uniformly(str(tmp_path / other))


def test_generated_paths_fall_back_to_avi(tmp_path):
    from asva_amd.evaluation import _generated_paths

    root = tmp_path / "gen"
    (root / "dog").mkdir(parents=True)
    for i in (1, 0):
        (root / "dog" / f"x_clip-0{i}.avi").write_bytes(b"")
    assert _generated_paths(str(root), "dog/x.mp4") == [f"{root}/dog/x_clip-00.avi", f"{root}/dog/x_clip-01.avi"]
    assert _generated_paths(str(root), "dog/x.avi") == [f"{root}/dog/x_clip-00.avi", f"{root}/dog/x_clip-01.avi"]
    assert _generated_paths(str(root), "dog/y.mp4") == []
    (root / "dog" / "x_clip-00.mp4").write_bytes(b"")
    assert _generated_paths(str(root), "dog/x.mp4") == [f"{root}/dog/x_clip-00.mp4"]       # the groundtruth's extension is preferred


def test_decoder_setting(monkeypatch):
    from asva_amd import video_io as V

    assert V.get_jpeg_decoder() == "host"                                  # the default
    with pytest.raises(ValueError, match="unknown mode"):
        V.set_jpeg_decoder("gpu")
    with pytest.raises(ValueError, match="unknown mode"):
        V._decoder_from_env({"AVSD_JPEG_DECODER": "gpu"})
    V._decoder_from_env({})
    V._decoder_from_env({"AVSD_JPEG_DECODER": "host"})
    assert V.get_jpeg_decoder() == "host"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)           # as on a machine without a GPU
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.set_jpeg_decoder("device")
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V._decoder_from_env({"AVSD_JPEG_DECODER": "device"})
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.decode_jpeg_frames([_pil_encode(_image(8, 8))])
    with pytest.raises(RuntimeError, match="needs the GPU"):
        V.decode_mjpeg_frames([_pil_encode(_image(8, 8))], decoder="device")
    with pytest.raises(ValueError, match="unknown decoder"):
        V.decode_mjpeg_frames([_pil_encode(_image(8, 8))], decoder="gpu")
    assert V.get_jpeg_decoder() == "host"


def test_read_mjpeg_avi_defaults_return_what_they_returned(tmp_path):
    """the reader before the split: every 00dc chunk through PIL, stacked, a host tensor; PCM / 32767"""
    from asva_amd import video_io as V

    frames, audio = _id_clip()
    path = V.write_mjpeg_avi(str(tmp_path / "v.avi"), frames[:5], 6.0, audio, 16000)
    video, fps, a, afps = V.read_mjpeg_avi(path)
    jpegs, fps_w, pcm, nch, afps_w = V.walk_mjpeg_avi(path)
    assert len(jpegs) == 5 and (fps_w, nch, afps_w) == (6.0, 1, 16000) and fps == 6.0 and afps == 16000
    assert video.dtype == torch.uint8 and not video.is_cuda and torch.equal(video, torch.from_numpy(np.stack([_pil_decode(j) for j in jpegs])))
    assert jpegs == [_pil_encode(f, quality=95) for f in frames[:5]]
    want = (np.clip(audio.T.astype(np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")
    assert pcm == want.tobytes() and torch.equal(a, torch.from_numpy(want.T.astype(np.float32) / 32767.0))
    silent = V.write_mjpeg_avi(str(tmp_path / "s.avi"), frames[:2], 6.0)
    assert V.read_mjpeg_avi(silent)[2] is None
    assert os.path.getsize(silent) < os.path.getsize(path)
