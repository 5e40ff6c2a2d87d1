"""The on-device baseline JPEG decoder (asva_amd/csrc/jpeg.hip: avsd_jpeg_decode_scan, avsd_jpeg_idct_rgb_u8) on the MI355X, and its
wiring into video_io.decode_jpeg_frames, read_mjpeg_avi, the clip loaders and the evaluation driver.

Everything is exact.  Coefficients: equal to the sequential Python decoder of tests/jpeg_dec_ref.py, at a subsequence length of 128
bits and at the default.  Pixels: equal to PIL's decode of the same bytes.  A damaged stream is refused by name and leaves the
decoder usable."""
import io
import warnings

import numpy as np
import pytest
import torch

from tests import jpeg_dec_ref as D
from tests import jpeg_ref as R
from tests.helpers import load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUBSEQ = (128, None)              # the shortest allowed, and the default (ops.JPEG_SUBSEQ_BITS)


def _pil_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _pil_encode(img, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _image(H, W, seed=5):
    rng = np.random.default_rng(seed)
    base = R.smooth_image(max(H, 8), max(W, 8))[:H, :W].astype(np.int64)
    return np.clip(base + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _check_coefficients(jpegs, what):
    """the device's coefficients of `jpegs` (one call) against the sequential decoder, at both subsequence lengths"""
    from asva_amd import video_io as V

    want = np.stack([D.decode_scan(D.parse(j)) for j in jpegs])
    for s in SUBSEQ:
        counters = {}
        got = V.decode_jpeg_coefficients(jpegs, DEV, subseq_bits=s, counters=counters)
        assert got.dtype == torch.int16 and got.is_cuda and tuple(got.shape) == want.shape, (what, s, got.shape, want.shape)
        print(f"  {what}, subsequences of {s or 'default'} bits: re-decoding rounds {counters['rounds']}")
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (what, s)
    return want


def test_one_mcu_is_shorter_than_a_subsequence():
    data = R.encode(R.named_frames()["mcu"], 95)
    assert 8 * len(D.parse(data)["scan"]) > 128                             # several lanes at 128 bits
    _check_coefficients([data], "one MCU, q 95")
    flat = R.encode(R.named_frames()["flat"][:, :8], 50)
    assert 8 * len(D.parse(flat)["scan"]) < 128                             # one lane at either length
    _check_coefficients([flat], "one flat MCU")


def test_handmade_coefficients():
    """ZRL runs, coefficient 63 set, no EOB, the largest categories, the longest block there is"""
    qy, qc = R.tables(95)
    for name, coef in R.handmade_coefficients().items():
        data = R.jpeg_from_coefficients(coef, coef.shape[0] * 8, coef.shape[1] * 8, qy, qc)
        want = _check_coefficients([data], name)
        assert np.array_equal(want[0].reshape(coef.shape), coef), name


def test_device_round_trip_of_the_packer():
    """ops.jpeg_pack's output fed straight back, without a copy to the host: the coefficients return"""
    from asva_amd import ops
    from asva_amd import video_io as V

    rng = np.random.default_rng(2)
    coef = np.zeros((3, 4, 5, 3, 64), dtype=np.int16)                        # three frames of 4 x 5 MCUs
    coef[..., 0] = rng.integers(-200, 200, coef.shape[:-1])
    keep = rng.random(coef[..., 1:].shape) < 0.15
    coef[..., 1:] = np.where(keep, rng.integers(-40, 41, keep.shape), 0)
    coef[1, ..., 1:] = np.where(rng.random(keep.shape[1:]) < 0.9, rng.integers(-1023, 1024, keep.shape[1:]), 0)      # a dense frame
    coef_d = torch.from_numpy(coef).to(DEV)
    stream, nbytes = ops.jpeg_pack(coef_d)
    spec = {tc_th: (bits, vals) for tc_th, bits, vals in V._DHT}
    words = np.concatenate([V.huffman_decode_table(*spec[(0x10 if ac else 0x00) | (1 if comp else 0)], dc=not ac) for comp in range(3)
                            for ac in (0, 1)])
    tables = torch.from_numpy(words.view(np.int32))[None].to(DEV)
    offsets = torch.arange(3, device=DEV, dtype=torch.int64) * stream.stride(0)
    for s in (128, ops.JPEG_SUBSEQ_BITS):
        got, status = ops.jpeg_decode_scan(stream.view(-1), offsets, nbytes * 8, torch.zeros(3, dtype=torch.int32, device=DEV), tables, 60, "444",
                                           subseq_bits=s)
        assert status.tolist() == [0, 0, 0], (s, status.tolist())
        assert torch.equal(got.view(coef_d.shape), coef_d), s


def test_flat_and_busy_halves():
    """a frame whose upper half is flat grey (about a hundred blocks inside one subsequence) and whose lower half is noise (several
    subsequences per block), and the opposite"""
    img = np.full((64, 64, 3), 128, dtype=np.uint8)
    img[32:] = _noise(32, 64, 3)
    for name, frame in (("flat then noise", img), ("noise then flat", img[::-1].copy())):
        _check_coefficients([R.encode(frame, 95)], f"{name}, 4:4:4")
        _check_coefficients([_pil_encode(frame, quality=95)], f"{name}, 4:2:0")


def test_blocks_longer_than_a_subsequence():
    from asva_amd import video_io as V

    data = R.encode(_noise(32, 32, 7), 100)
    info = V.parse_jpeg(data)
    n_blocks, n_bits = 16 * 3, 8 * len(D.parse(data)["scan"])
    assert n_bits > 2 * 128 * n_blocks          # more than twice as many 128-bit lanes as blocks: some block is longer than 128 bits
    assert b"\xff\x00" in info["scan"]           # and the stream holds stuffing
    _check_coefficients([data], "32 x 32 noise, q 100")


def test_three_frames_of_different_lengths_and_tables_in_one_call():
    imgs = [_image(40, 56, seed=1), _noise(40, 56, 4), _image(40, 56, seed=2)]
    jpegs = [_pil_encode(imgs[0], quality=50), _pil_encode(imgs[1], quality=95), _pil_encode(imgs[2], quality=75, optimize=True)]
    infos = [D.parse(j) for j in jpegs]
    assert len({len(i["scan"]) for i in infos}) == 3 and infos[0]["qtabs"] != infos[1]["qtabs"] and infos[2]["ac"] != infos[0]["ac"]
    _check_coefficients(jpegs, "q 50 | q 95 | optimize")


def test_420_at_40x56():
    _check_coefficients([_pil_encode(_image(40, 56), quality=90)], "4:2:0, 40 x 56")


# ---- pixels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", (50, 95))
def test_pixels_of_device_encoded_444(quality):
    from asva_amd import video_io as V

    jpegs = V.encode_jpeg_frames(R.clip_frames(), quality)                  # (3, 48, 64, 3)
    got = V.decode_jpeg_frames(jpegs, DEV)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (3, 48, 64, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack([_pil_decode(j) for j in jpegs]))


@pytest.mark.parametrize("size", ((48, 64), (40, 56), (37, 51), (256, 256)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("quality", (50, 95))
def test_pixels_of_pil_420(size, quality):
    from asva_amd import video_io as V

    n = 1 if size[0] == 256 else 2
    jpegs = [_pil_encode(_image(*size, seed=5 + t), quality=quality) for t in range(n)]
    assert D.parse(jpegs[0])["sampling"] == "420"
    want = np.stack([_pil_decode(j) for j in jpegs])
    for s in SUBSEQ:
        got = V.decode_jpeg_frames(jpegs, DEV, subseq_bits=s)
        assert tuple(got.shape) == (n, *size, 3)
        diff = np.abs(got.cpu().numpy().astype(np.int64) - want)
        print(f"  {size} q {quality}, subsequences of {s or 'default'} bits: {int((diff != 0).sum())} of {diff.size} bytes differ, max {int(diff.max())}")
        assert int(diff.max()) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_cut_scan_is_refused_by_name_and_the_decoder_stays_usable():
    from asva_amd import video_io as V

    jpegs = [_pil_encode(_image(40, 56, seed=t), quality=90) for t in range(3)]
    info = V.parse_jpeg(jpegs[1])
    head = jpegs[1][:jpegs[1].index(info["scan"])]
    half = info["scan"][:len(info["scan"]) // 2]
    if half.endswith(b"\xff"):
        half = half[:-1]
    cut = head + half + b"\xff\xd9"
    assert V.parse_jpeg(cut)["scan"] == half                                # the markers are whole: only the device can tell
    for s in SUBSEQ:
        with pytest.raises(ValueError, match="frame 1 did not decode"):
            V.decode_jpeg_frames([jpegs[0], cut, jpegs[2]], DEV, subseq_bits=s)
    with pytest.raises(ValueError, match="frame 0 did not decode"):
        V.decode_jpeg_frames([cut], DEV)
    got = V.decode_jpeg_frames(jpegs, DEV)
    assert np.array_equal(got.cpu().numpy(), np.stack([_pil_decode(j) for j in jpegs]))


def test_refused_formats_fall_back_to_pil_with_one_warning(monkeypatch):
    from PIL import Image

    from asva_amd import video_io as V

    img = _image(40, 56)
    buf = io.BytesIO()
    Image.fromarray(img).convert("L").save(buf, format="JPEG")
    files = [_pil_encode(img, progressive=True), buf.getvalue(), _pil_encode(img, subsampling=1)]
    monkeypatch.setattr(V, "_warned_format", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for f in files:
            with pytest.raises(ValueError, match="parse_jpeg"):
                V.decode_jpeg_frames([f], DEV)
            got = V.decode_mjpeg_frames([f], decoder="device")
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), _pil_decode(f)[None])
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning) and "device JPEG decoder" in str(w.message)]) == 1


# ---- readers ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def device_decoder():
    from asva_amd import video_io as V

    V.set_jpeg_decoder("device")
    yield
    V.set_jpeg_decoder("host")


def _id_clip():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 255, (60, 48, 64, 3), dtype=np.uint8)
    frames[:, :16, :16] = (4 * np.arange(60, dtype=np.uint8))[:, None, None, None]
    audio = (rng.standard_normal((1, 32000)) * 0.1).astype(np.float32)
    return frames, audio


def test_read_mjpeg_avi_on_the_device_equals_the_host(tmp_path):
    from asva_amd import video_io as V

    frames, audio = _id_clip()
    for encoder in ("device", "host"):
        path = V.write_mjpeg_avi(str(tmp_path / f"{encoder}.avi"), frames[:6], 6.0, audio, 16000, encoder=encoder)
        host = V.read_mjpeg_avi(path)
        dev = V.read_mjpeg_avi(path, decoder="device")
        assert dev[0].is_cuda and not host[0].is_cuda and torch.equal(dev[0].cpu(), host[0]), encoder
        assert dev[1] == host[1] and torch.equal(dev[2], host[2]) and dev[3] == host[3]


def test_clip_loaders_on_the_device(tmp_path, device_decoder):
    from asva_amd import video_io as V
    from asva_amd.data_utils import _open_video, load_av_clips_uniformly

    frames, audio = _id_clip()
    path = V.write_mjpeg_avi(str(tmp_path / "v.avi"), frames, 30.0, audio, 16000)
    src = _open_video(path)
    on_device = src.video_clip(0.0, 1.0, 6, 6)
    late = src.video_clip(1.5, 1.0, 6, 6)                                   # runs past the end: the last frame is repeated
    V.set_jpeg_decoder("host")
    assert on_device.is_cuda and torch.equal(on_device.cpu(), src.video_clip(0.0, 1.0, 6, 6)) and torch.equal(late.cpu(), src.video_clip(1.5, 1.0, 6, 6))
    V.set_jpeg_decoder("device")
    vid, aud = load_av_clips_uniformly(path, video_fps=6, video_num_frame=6, image_size=(48, 64), num_clips=2, load_audio_as_melspectrogram=False)
    assert vid.is_cuda and vid.shape == (2, 6, 3, 48, 64) and vid.dtype == torch.float32 and len(aud) == 2 and aud[0].shape == (1, 16000)
    assert ((vid[0, :, :, 4, 4] * 255).mean(dim=1) / 4).round().int().tolist() == [0, 5, 10, 15, 20, 25]


def test_evaluation_over_avi_clips(tmp_path, device_decoder):
    """evaluate_generation_results over groundtruth and generated .avi files, decoded on the device: it completes and names every clip"""
    from asva_amd import avsync as A
    from asva_amd import fid
    from asva_amd import video_io as V
    from avgen.evaluations.eval import evaluate_generation_results
    from tests import avsync_ref as AR
    from tests import inception_ref as IR

    g = load_golden("avsync_tiny.pt")
    sync = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    sync.load_state_dict(AR.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"]))
    gf = load_golden("fid/fid_tiny.pt")
    inception = fid.InceptionV3((3,))
    inception.load_state_dict(IR.draw_state_dict(load_shapes("fid/state_dict_shapes.json"), gf["seed"]))
    rng = np.random.default_rng(0)
    (tmp_path / "gt").mkdir()
    (tmp_path / "gen").mkdir()
    names = ["beta.avi", "alpha.avi"]                                          # unsorted: the driver sorts
    for n in names:
        frames = np.repeat(np.repeat(rng.integers(0, 255, (12, 12, 12, 3), dtype=np.uint8), 8, 1), 8, 2)       # 2 s at 6 fps, 96 x 96
        audio = (rng.standard_normal((1, 2 * 16000)) * 0.1).astype(np.float32)
        V.write_mjpeg_avi(str(tmp_path / "gt" / n), frames, 6.0, audio, 16000)
        for k in range(2):                                                    # one clip written by PIL (4:2:0), one by the device (4:4:4)
            gen = np.repeat(np.repeat(rng.integers(0, 255, (3, 6, 6, 3), dtype=np.uint8), 16, 1), 16, 2)
            V.write_mjpeg_avi(str(tmp_path / "gen" / f"{n[:-4]}_clip-{k:02d}.avi"), gen, 6.0, (rng.standard_normal((1, 8000)) * 0.1).astype(np.float32),
                              16000, encoder="device" if k else "host")
    res = evaluate_generation_results(groundtruth_video_root=str(tmp_path / "gt"), groundtruth_video_names=list(names),
                                      groundtruth_categories=["dog", "cat"], num_clips_per_video=2, generated_video_root=str(tmp_path / "gen"),
                                      result_save_path=str(tmp_path / "results" / "metrics.json"), image_size=96, video_fps=6, video_num_frame=3,
                                      eval_fid=True, eval_fvd=False, eval_clipsim=False, eval_relsync=True, eval_alignsync=False,
                                      record_instance_metrics=True, models={"fid": inception, "avsync": sync})
    assert list(res["instance_metrics"]) == ["alpha_clip-00.avi", "alpha_clip-01.avi", "beta_clip-00.avi", "beta_clip-01.avi"]
    assert np.isfinite(res["FID"]) and res["FID"] > 0.0 and np.isfinite(res["RelSync_mean"])
