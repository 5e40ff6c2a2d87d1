"""Whole-track animation, host side (-m "not gpu"): the window arithmetic of data_utils.track_windows against known answers and
exact rational arithmetic, and the streaming Motion-JPEG writer video_io.MjpegAviWriter read back by read_mjpeg_avi."""
import io
import struct
from fractions import Fraction
from math import ceil

import numpy as np
import pytest
import torch

from asva_amd.data_utils import track_windows
from asva_amd.video_io import MjpegAviWriter, read_mjpeg_avi, walk_mjpeg_avi


# ---- track_windows ---------------------------------------------------------------------------------------------------------
def test_exactly_one_window():
    windows, W, n_frames, padded = track_windows(32000)
    assert (windows, W, n_frames, padded) == ([(0, 0)], 1, 12, 32000)


def test_one_sample_more_opens_a_second_window():
    windows, W, n_frames, padded = track_windows(32001)
    # window 1 starts at frame 11 = sample 11 * 16000 / 6 = 29333.3 -> 29333; 32001 samples are 12.0004 frame periods -> 13 frames
    assert windows == [(0, 0), (29333, 11)] and W == 2 and n_frames == 13 and padded == 29333 + 32000


def test_ten_seconds():
    windows, W, n_frames, padded = track_windows(160000, 16000, 6, 12)
    # 128000 samples beyond the first window, 29333.3 per hop -> 4.36 -> 5 more windows; 10 s at 6 fps = 60 frames of the 67 made
    assert W == 6 and n_frames == 60
    assert windows == [(0, 0), (29333, 11), (58666, 22), (88000, 33), (117333, 44), (146666, 55)]
    assert padded == 146666 + 32000 and padded >= 160000


def test_shorter_than_one_window_is_padded_to_one():
    for n in (0, 1, 16000, 31999):
        windows, W, n_frames, padded = track_windows(n)
        assert (windows, W, n_frames, padded) == ([(0, 0)], 1, 12, 32000)


def test_24_frames_at_12_fps():
    windows, W, n_frames, padded = track_windows(5 * 16000, 16000, 12, 24)
    # window 32000 samples, hop 23 * 16000 / 12 = 30666.7: 48000 beyond the first window -> 1.57 -> 2 more windows; 5 s = 60 frames
    assert W == 3 and n_frames == 60 and windows == [(0, 0), (30666, 23), (61333, 46)] and padded == 61333 + 32000
    assert track_windows(32000, 16000, 12, 24)[1:3] == (1, 24)


@pytest.mark.parametrize("sr,fps,F", [(16000, 6, 12), (16000, 12, 24), (44100, 7, 5), (22050, 25, 2), (16000, 6, 4)])
def test_starts_are_the_floor_of_the_exact_rational_time(sr, fps, F):
    hop = Fraction((F - 1) * sr, fps)
    win = F * sr // fps
    n = int(1000 * hop) + win                                        # long enough for windows 0 .. 1000
    windows, W, n_frames, padded = track_windows(n, sr, fps, F)
    assert W >= 1001 and len(windows) == W
    for k, (s, first) in enumerate(windows):
        exact = k * hop
        assert s == exact.numerator // exact.denominator and first == k * (F - 1)
    # W and n_frames by the formulas in exact arithmetic
    assert W == 1 + ceil(Fraction(max(0, n - win)) / hop)
    assert n_frames == min(1 + W * (F - 1), max(F, ceil(Fraction(n * fps, sr))))
    assert padded == windows[-1][0] + win >= n                       # the last window reaches the end of the track ...
    assert W == 1 or windows[-2][0] + win < n                        # ... and the one before it does not


@pytest.mark.parametrize("n", [0, 31999, 32000, 32001, 61333, 61334, 160000, 999983])
def test_consecutive_windows_share_exactly_one_frame(n):
    F = 12
    windows, W, n_frames, _ = track_windows(n, 16000, 6, F)
    frames = [set(range(first, first + F)) for _, first in windows]
    for a, b in zip(frames, frames[1:]):
        assert len(a & b) == 1 and max(a) == min(b)
    for a, c in zip(frames, frames[2:]):
        assert not a & c
    assert set().union(*frames) == set(range(1 + W * (F - 1))) and F <= n_frames <= 1 + W * (F - 1)
    assert W == 1 or n_frames > 1 + (W - 1) * (F - 1)                # every window contributes a frame of its own


def test_bad_arguments():
    for bad in ((-1, 16000, 6, 12), (100, 0, 6, 12), (100, 16000, 0, 12), (100, 16000, 6, 1)):
        with pytest.raises(ValueError, match="track_windows"):
            track_windows(*bad)


# ---- MjpegAviWriter ----------------------------------------------------------------------------------------------------------
def _pil_roundtrip(frames, quality=95):
    from PIL import Image

    out = []
    for fr in frames:
        buf = io.BytesIO()
        Image.fromarray(fr).save(buf, format="JPEG", quality=quality)
        out.append(np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
    return np.stack(out)


def test_appended_file_reads_back(tmp_path):
    rng = np.random.default_rng(0)
    H, W = 24, 40
    pieces = [rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8) for n in (12, 11, 11)]
    audio = torch.from_numpy(rng.uniform(-1, 1, size=(1, 34 * 16000 // 6)).astype(np.float32))
    path = str(tmp_path / "track.avi")
    w = MjpegAviWriter(path, 6, (H, W), 16000, encoder="host")
    assert [w.append(pieces[0]), w.append(torch.from_numpy(pieces[1])), w.append(pieces[2])] == [12, 23, 34]
    assert w.close(audio) == path
    video, fps, aud, afps = read_mjpeg_avi(path, decoder="host")
    assert video.shape == (34, H, W, 3) and video.dtype == torch.uint8 and fps == 6.0 and afps == 16000
    assert np.array_equal(video.numpy(), _pil_roundtrip(np.concatenate(pieces)))
    pcm = (audio.numpy().astype(np.float64) * 32767.0).round()                                      # the writer's 16-bit PCM
    assert aud.shape == audio.shape and np.array_equal(aud.numpy(), (pcm / 32767.0).astype(np.float32))

    # headers: RIFF size, frame counts of avih and of the video stream, the largest frame, the audio length, the index
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    jpegs, _, pcm_bytes, nch, _ = walk_mjpeg_avi(path)
    assert len(jpegs) == 34 and nch == 1 and len(pcm_bytes) == 2 * audio.shape[1]
    avih = data.index(b"avih") + 8
    us_per_frame, _, _, flags, total_frames, _, streams, max_frame, width, height = struct.unpack("<10I", data[avih:avih + 40])
    assert (us_per_frame, flags, total_frames, streams, width, height) == (166667, 0x10, 34, 2, W, H)
    assert max_frame == max(len(j) for j in jpegs)
    strh_v = data.index(b"strh") + 8
    assert data[strh_v:strh_v + 8] == b"vidsMJPG" and struct.unpack("<I", data[strh_v + 32:strh_v + 36])[0] == 34     # dwLength
    strh_a = data.index(b"strh", strh_v) + 8
    assert data[strh_a:strh_a + 4] == b"auds" and struct.unpack("<I", data[strh_a + 32:strh_a + 36])[0] == audio.shape[1]
    movi = data.index(b"movi")
    assert data[movi - 8:movi - 4] == b"LIST"
    idx = data.index(b"idx1", movi + struct.unpack("<I", data[movi - 4:movi])[0] - 4)
    n_idx = struct.unpack("<I", data[idx + 4:idx + 8])[0]
    assert n_idx == 16 * 35 and idx + 8 + n_idx == len(data)
    for i in range(35):
        tag, fl, off, size = struct.unpack("<4sIII", data[idx + 8 + 16 * i:idx + 24 + 16 * i])
        want = jpegs[i] if i < 34 else pcm_bytes
        assert tag == (b"00dc" if i < 34 else b"01wb") and fl == 0x10 and size == len(want)
        assert data[movi + off:movi + off + 8] == tag + struct.pack("<I", size) and data[movi + off + 8:movi + off + 8 + size] == want


def test_file_without_audio_and_misuse(tmp_path):
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, size=(3, 16, 16, 3), dtype=np.uint8)
    path = str(tmp_path / "silent.avi")
    with MjpegAviWriter(path, 6, (16, 16), encoder="host") as w:
        w.append(frames)
        with pytest.raises(ValueError, match=r"\(T, 16, 16, 3\)"):
            w.append(frames[:, :8])
    video, fps, aud, _ = read_mjpeg_avi(path, decoder="host")
    assert aud is None and fps == 6.0 and np.array_equal(video.numpy(), _pil_roundtrip(frames))
    data = open(path, "rb").read()
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8 and b"JUNK" in data[:data.index(b"movi")]
    avih = data.index(b"avih") + 8
    assert struct.unpack("<10I", data[avih:avih + 40])[4:7:2] == (3, 1)                              # 3 frames, 1 stream
    with pytest.raises(ValueError, match="closed"):
        w.append(frames)
    with pytest.raises(ValueError, match="no frames"):
        MjpegAviWriter(str(tmp_path / "empty.avi"), 6, (16, 16)).close()


def test_write_mjpeg_avi_and_the_writer_hold_the_same_streams(tmp_path):
    """one call or three pieces: the same compressed frames and the same PCM, in the same order"""
    from asva_amd.video_io import write_mjpeg_avi

    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, size=(5, 16, 24, 3), dtype=np.uint8)
    audio = rng.uniform(-1, 1, size=(2, 4000)).astype(np.float32)
    a, b = str(tmp_path / "a.avi"), str(tmp_path / "b.avi")
    write_mjpeg_avi(a, frames, 6, audio, 16000, encoder="host")
    w = MjpegAviWriter(b, 6, (16, 24), 16000, encoder="host")
    w.append(frames[:2])
    w.append(frames[2:])
    w.close(audio)
    assert walk_mjpeg_avi(a) == walk_mjpeg_avi(b)
