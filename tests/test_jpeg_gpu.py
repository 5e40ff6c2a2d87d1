"""The on-device baseline JPEG encoder (asva_amd/csrc/jpeg.hip: avsd_jpeg_quantize_u8, avsd_jpeg_pack_i16) on the MI355X
against the float64 / Python-integer reference of tests/jpeg_ref.py and against libjpeg's decoder through PIL, and its wiring
into video_io.encode_jpeg_frames, write_mjpeg_avi and the pipeline's "uint8_device" frames.

Quantiser: the coefficients equal the reference's, except where the reference's pre-rounding quotient lies within 4e-3 of a
tie (jpeg_ref.TIE_WINDOW: the worst-case f32 error of a 64-term sum of values up to 1024 at a table entry of 1,
64 x 1024 x 2^-24), where they may differ by exactly 1.  Entropy coder: byte-exact.  Decoded pixels: within the libjpeg bound
stored in tests/golden/jpeg/meta.json of the float64 reconstruction of the device's own coefficients."""
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R
from tests.helpers import ROOT, filled_unet, load_golden
from tests.test_host_cpu import TINY_VAE, _filled_vae

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMED = R.named_frames()
with open(os.path.join(ROOT, "tests", "golden", "jpeg", "meta.json")) as _f:
    BOUND = json.load(_f)["libjpeg_bound_levels"]


def _tables_d(quality):
    qy, qc = R.tables(quality)
    return qy, qc, torch.tensor(qy, dtype=torch.int16, device=DEV), torch.tensor(qc, dtype=torch.int16, device=DEV)


def _quantize(frames, quality):
    from asva_amd import ops

    _qy, _qc, qy_d, qc_d = _tables_d(quality)
    return ops.jpeg_quantize(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), qy_d, qc_d)


def _decode(data):
    from PIL import Image

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return np.asarray(im.convert("RGB"))


def _check_coefficients(got, frame, quality, what):
    qy, qc = R.tables(quality)
    quot = R.quotients(frame, qy, qc)
    ref, tie = R.round_half_away(quot), R.near_tie(quot)
    assert float(tie.mean()) <= 0.02, (what, float(tie.mean()))             # the cap on the reference side
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = np.abs(got - ref)
    print(f"  {what}: {int((diff != 0).sum())} of {diff.size} coefficients differ ({int(tie.sum())} within the tie window), max |diff| {int(diff.max())}")
    assert np.array_equal(got[~tie], ref[~tie]), what
    assert int(diff[tie].max(initial=0)) <= 1, what


@pytest.mark.parametrize("name,quality", R.quantize_cases(), ids=lambda v: str(v))
def test_quantize_matches_float64_reference(name, quality):
    coef = _quantize(NAMED[name][None], quality)
    assert coef.dtype == torch.int16 and coef.is_cuda
    _check_coefficients(coef[0], NAMED[name], quality, f"{name} q{quality}")
    if name == "flat":
        assert int(coef[..., 1:].abs().max()) == 0                         # a flat frame has no AC at all


def test_quantize_batch_equals_single_calls():
    frames = R.clip_frames()
    batch = _quantize(frames, 95)
    assert batch.shape == (3, 6, 8, 3, 64)
    for t in range(3):
        assert torch.equal(batch[t:t + 1], _quantize(frames[t:t + 1], 95)), t
        _check_coefficients(batch[t], frames[t], 95, f"clip frame {t}")
    assert not torch.equal(batch[0], batch[2])


def _pack_inputs():
    """{name: int16 (n, rows, cols, 3, 64)}: reference coefficients of the named frames, the hand-made corner cases, the residue
    sweep, and batches of different content in one call"""
    out = {}
    for name, q in (("mcu", 100), ("noise", 100), ("noise", 95), ("smooth", 95), ("smooth", 75), ("flat", 95), ("checker", 95)):
        out[f"{name}_q{q}"] = R.quantize(NAMED[name], *R.tables(q)).astype(np.int16)[None]
    for name, c in R.handmade_coefficients().items():
        out[name] = c[None]
    out["residues"] = np.stack(R.residue_sweep())                             # 8 single-MCU frames in one call
    clip = np.stack([R.quantize(f, *R.tables(95)) for f in R.clip_frames()]).astype(np.int16)
    out["clip"] = clip
    out["clip_reversed"] = clip[::-1].copy()
    return out


def _pack(coef):
    from asva_amd import ops

    stream, nbytes = ops.jpeg_pack(torch.from_numpy(np.ascontiguousarray(coef)).to(DEV))
    counts = nbytes.cpu().tolist()
    host = stream.cpu().numpy()
    return [host[t, :counts[t]].tobytes() for t in range(len(counts))]


def test_pack_is_byte_exact():
    stuffed, residues = 0, set()
    for name, coef in _pack_inputs().items():
        got = _pack(coef)
        assert len(got) == coef.shape[0]
        for t, g in enumerate(got):
            ref, nbits = R.encode_scan(coef[t])
            residues.add(nbits % 8)
            assert len(g) == len(ref) == (nbits + 7) // 8, (name, t, len(g), len(ref))
            assert g == ref, (name, t, next(i for i in range(len(ref)) if g[i] != ref[i]))
            stuffed += len(g.replace(b"\xff", b"\xff\x00")) - len(g)
    assert stuffed > 0 and residues == set(range(8)), (stuffed, residues)


def test_pack_is_deterministic_and_the_same_in_both_builds():
    from asva_amd import precision

    inputs = _pack_inputs()
    frames = R.clip_frames()
    outs = {}
    for build in ("bf16", "fp16"):
        precision.set_precision(build)
        try:
            for rep in range(2):
                outs[build, rep] = ({k: _pack(v) for k, v in inputs.items()}, _quantize(frames, 95).cpu())
        finally:
            precision.set_precision("bf16")
    first = outs["bf16", 0]
    for key, (streams, coef) in outs.items():
        assert streams == first[0], key
        assert torch.equal(coef, first[1]), key


def _check_decoded(jpegs, frames, coef, quality, what):
    """every stream decodes; pixels within the libjpeg bound of the float64 reconstruction of the DEVICE's coefficients; PSNR
    against the source at least the reference encoder's minus 0.01 dB (only tie flips separate the two)"""
    qy, qc = R.tables(quality)
    coef = coef.cpu().numpy()
    for t, data in enumerate(jpegs):
        dec = _decode(data)
        assert dec.shape == frames[t].shape
        err = float(np.abs(dec.astype(np.float64) - R.reconstruct(coef[t], qy, qc)).max())
        ours, ref = R.psnr(dec, frames[t]), R.psnr(_decode(R.encode(frames[t], quality)), frames[t])
        print(f"  {what} frame {t}: {len(data)} bytes, max |decoded - reconstruction| {err:.3f} levels (bound {BOUND}), PSNR {ours:.3f} dB (reference {ref:.3f})")
        assert err <= BOUND, (what, t, err)
        assert ours >= ref - 0.01, (what, t, ours, ref)


def test_encode_jpeg_frames_end_to_end():
    from asva_amd import video_io as V

    frames = R.clip_frames()
    dev = torch.from_numpy(frames).to(DEV)
    jpegs = V.encode_jpeg_frames(dev, quality=95)
    assert len(jpegs) == 3 and all(j[:2] == b"\xff\xd8" and j[-2:] == b"\xff\xd9" for j in jpegs)
    _check_decoded(jpegs, frames, _quantize(frames, 95), 95, "encode_jpeg_frames")
    assert V.encode_jpeg_frames(frames, quality=95) == jpegs                # a host array is uploaded first
    for bad in (dev[:, :47], dev[..., :2], dev.float(), dev[0]):
        with pytest.raises(ValueError):
            V.encode_jpeg_frames(bad)


def test_ops_and_entry_points_refuse_bad_arguments():
    from asva_amd import _lib, ops

    _qy, _qc, qy_d, qc_d = _tables_d(95)
    good = torch.zeros(1, 8, 16, 3, dtype=torch.uint8, device=DEV)
    assert ops.jpeg_quantize(good, qy_d, qc_d).shape == (1, 1, 2, 3, 64)
    for f, a, b in ((good.cpu(), qy_d, qc_d), (good, qy_d.cpu(), qc_d), (good.float(), qy_d, qc_d), (good, qy_d.float(), qc_d),
                    (good[..., :2], qy_d, qc_d), (good, qy_d[:63], qc_d), (good[:, :, ::2], qy_d, qc_d)):
        with pytest.raises(ValueError):
            ops.jpeg_quantize(f, a, b)
    for shape in ((1, 12, 16, 3), (1, 8, 20, 3)):                           # not whole MCUs: the library says so
        with pytest.raises(_lib.AvsdError, match="multiples of 8"):
            ops.jpeg_quantize(torch.zeros(shape, dtype=torch.uint8, device=DEV), qy_d, qc_d)
    coef = torch.zeros(1, 3, 64, dtype=torch.int16, device=DEV)
    assert ops.jpeg_pack(coef)[1].tolist() == [2]                           # 2 + 4, 2 + 2, 2 + 2 bits and two 1-bits of padding
    for bad in (coef.cpu(), coef.int(), coef[:, :2], coef[..., :63], coef[:, :, ::2]):
        with pytest.raises(ValueError):
            ops.jpeg_pack(bad)


def test_writer_with_the_device_encoder(tmp_path):
    from asva_amd import video_io as V

    frames = R.clip_frames()
    rng = np.random.default_rng(6)
    audio = torch.from_numpy((rng.standard_normal((2, 8000)) * 0.1).astype(np.float32))
    path = V.write_mjpeg_avi(str(tmp_path / "d.avi"), torch.from_numpy(frames).to(DEV), 6, audio, 16000, encoder="device")
    video, fps, aud, afps = V.read_mjpeg_avi(path)
    assert video.shape == (3, 48, 64, 3) and video.dtype == torch.uint8 and fps == 6.0 and afps == 16000
    assert aud.shape == (2, 8000) and float((aud - audio).abs().max()) <= 1.0 / 32767.0
    coef = _quantize(frames, 95).cpu().numpy()
    qy, qc = R.tables(95)
    for t in range(3):
        err = float(np.abs(video[t].numpy().astype(np.float64) - R.reconstruct(coef[t], qy, qc)).max())
        assert err <= BOUND, (t, err)
    # a host array is uploaded first and gives the same file; the setting selects the encoder when the argument is absent
    same = V.write_mjpeg_avi(str(tmp_path / "h.avi"), frames, 6, audio, 16000, encoder="device")
    assert open(same, "rb").read() == open(path, "rb").read()
    V.set_jpeg_encoder("device")
    try:
        assert V.get_jpeg_encoder() == "device"
        via_setting = V.write_mjpeg_avi(str(tmp_path / "s.avi"), frames, 6, audio, 16000)
    finally:
        V.set_jpeg_encoder("host")
    assert open(via_setting, "rb").read() == open(path, "rb").read()
    host = V.write_mjpeg_avi(str(tmp_path / "p.avi"), frames, 6, audio, 16000)
    assert open(host, "rb").read() != open(path, "rb").read()              # PIL's 4:2:0 frames are other bytes
    # sizes that are not whole MCUs go to PIL, with a warning
    odd = frames[:, :44, :60]
    V._warned_size = False
    with pytest.warns(RuntimeWarning, match="multiples of 8"):
        p_odd = V.write_mjpeg_avi(str(tmp_path / "o.avi"), torch.from_numpy(np.ascontiguousarray(odd)).to(DEV), 6, encoder="device")
    assert open(p_odd, "rb").read() == open(V.write_mjpeg_avi(str(tmp_path / "o2.avi"), odd, 6), "rb").read()


def test_pipeline_uint8_device_frames_are_the_uint8_frames(tmp_path):
    from asva_amd.pipeline import AudioCondAnimationPipeline, generate_videos
    from asva_amd.schedulers import PNDMScheduler
    from asva_amd import video_io as V

    g = load_golden("unet_tiny_e2e.pt")
    f, h, w = g["sample"].shape[2:]
    pipe = AudioCondAnimationPipeline(unet=filled_unet(g["config"]), scheduler=PNDMScheduler(), vae=_filled_vae(TINY_VAE))
    pipe.to("cuda")
    pipe.set_progress_bar_config(disable=True)
    gen = torch.Generator().manual_seed(0)
    il, noise = torch.randn(1, 4, h, w, generator=gen) * 0.18215, torch.randn(1, 4, f - 1, h, w, generator=gen)
    kw = dict(texts=[""], text_encodings=[g["text"][:1]], video_length=f, height=h * 8, width=w * 8, num_inference_steps=2,
              audio_guidance_scale=4.0, image_latents=il, audio_encodings=g["audio"][1:2], null_audio_encodings=g["audio"][:1],
              audio_masks=g["mask"], noise=noise, return_dict=False)
    host = pipe(**kw, output_type="uint8")
    dev = pipe(**kw, output_type="uint8_device")
    assert dev.is_cuda and not host.is_cuda and dev.dtype == torch.uint8 and dev.shape == (1, f, h * 8, w * 8, 3)
    assert torch.equal(dev.cpu(), host)
    # generate_videos hands device frames to the writer only when it writes files with the device encoder
    pipe.generation_steps = 2
    clips = [dict(image_latents=il[0], audio_encodings=g["audio"][1], null_audio_encodings=g["audio"][0])]
    gkw = dict(category="x", category_text_encoding=g["text"][:1], image_size=(h * 8, w * 8), video_num_frame=f, seed=5,
               device=torch.device("cuda"), clips=clips)
    seen = []
    V.set_jpeg_encoder("device")
    try:
        generate_videos(pipe, **gkw, save_template=str(tmp_path / "clip"), writer=lambda path, video, *a: seen.append(video))
        returned, _ = generate_videos(pipe, **gkw)
    finally:
        V.set_jpeg_encoder("host")
    assert len(seen) == 1 and seen[0].is_cuda and not returned[0].is_cuda and torch.equal(seen[0].cpu(), returned[0])
