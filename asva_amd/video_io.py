"""Codec-free video file writer / reader for the generation drivers.

The reference saves every generated clip with torchvision.io.write_video (H.264 + AAC in .mp4,
pipeline_audio_cond_animation.py:451-458).  Neither torchvision nor any H.264/AAC encoder exists in this image, so
`asva_amd.pipeline.write_video` falls back to this module: Motion-JPEG frames (PIL's JPEG encoder) + 16-bit PCM audio in a
RIFF/AVI container — playable by ffmpeg / VLC / OpenCV, and readable back here for the evaluation tools.  Same
arguments as the reference call: video (T, H, W, 3) uint8, fps, audio (C, Ta) float waveform in [-1, 1], audio_fps.

The frames can also be encoded on the device (`set_jpeg_encoder("device")`, $AVSD_JPEG_ENCODER, or `encoder="device"`):
`encode_jpeg_frames` runs the colour transform, DCT, quantiser and Huffman coder as kernels of the library (csrc/jpeg.hip)
and copies back the entropy-coded bytes instead of the raw frames; markers and FF byte stuffing are added here.  Those
streams are baseline JPEG, **4:4:4**, with the Annex K Huffman tables - not PIL's default 4:2:0 with the same quantisation
tables: the evaluation reads these files back, so the chroma is kept whole, and three planes of equal size keep the kernels
simple.  The default is "host": every byte this module writes is then PIL's.
"""
from __future__ import annotations

import io
import os
import struct
import warnings
from typing import List, Optional, Tuple

import numpy as np
import torch


def _chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _list(kind: bytes, payload: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


# ---- where the frames are encoded ----------------------------------------------------------------------------------------
_JPEG_ENCODERS = ("host", "device")
_jpeg_encoder = "host"
_NEEDS_GPU = ('the "device" JPEG encoder needs the GPU (torch.cuda.is_available() is False) and has no host path; '
              'use "host"')


def set_jpeg_encoder(mode: str) -> None:
    """Who encodes the frames `write_mjpeg_avi` stores.  "host": PIL, the default.  "device": `encode_jpeg_frames`
    (avsd_jpeg_quantize_u8 + avsd_jpeg_pack_i16); needs a GPU.  Read once from $AVSD_JPEG_ENCODER at import."""
    global _jpeg_encoder
    if mode not in _JPEG_ENCODERS:
        raise ValueError(f"set_jpeg_encoder: unknown mode {mode!r}; one of {_JPEG_ENCODERS}")
    if mode == "device" and not torch.cuda.is_available():
        raise RuntimeError(f'set_jpeg_encoder("device"): {_NEEDS_GPU}')
    _jpeg_encoder = mode


def get_jpeg_encoder() -> str:
    return _jpeg_encoder


def _encoder_from_env(environ=os.environ) -> None:
    if environ.get("AVSD_JPEG_ENCODER"):
        set_jpeg_encoder(environ["AVSD_JPEG_ENCODER"])


_encoder_from_env()

# ---- baseline JPEG: tables and markers (ITU-T T.81 Annex K, JFIF 1.01) ------------------------------------------------------
# natural (row-major) index of the coefficient at each zigzag position
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
            103, 99)
_K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
              99) + (99,) * 32
# Huffman table specifications K.3 - K.6 as (BITS, HUFFVAL); csrc/jpeg.hip codes with the same four
_AC_K5 = bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
                       "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
                       "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_K6 = bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738"
                       "393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6"
                       "a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
_DHT = (
    (0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
    (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)), _AC_K5),
    (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
    (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _AC_K6),
)


def jpeg_tables(quality: int) -> Tuple[List[int], List[int]]:
    """(luminance, chrominance) quantisation tables of libjpeg at `quality`, 64 entries each in natural (row-major) order: the
    Annex K tables scaled by s = 5000 // q below 50, else 200 - 2 q, as (base * s + 50) // 100 clamped to 1..255.  These are the
    tables PIL writes (and reports) for the same `quality`."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg_tables: quality must be in 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(255, max(1, (b * s + 50) // 100)) for b in base] for base in (_K1_LUMA, _K2_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def _jpeg_header(H: int, W: int, qy, qc) -> bytes:
    """SOI, APP0 (JFIF 1.01), DQT x 2, SOF0 (three components, 1 x 1 sampling each), DHT x 4, SOS"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((qy, qc)):
        out += _segment(0xDB, bytes((i,)) + bytes(q[n] for n in _ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes((1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, bits, vals in _DHT:
        out += _segment(0xC4, bytes((tc_th,)) + bits + vals)
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


_table_cache = {}


def _device_tables(quality: int, device):
    key = (int(quality), str(device))
    if key not in _table_cache:
        qy, qc = jpeg_tables(quality)
        # uint16 values in an int16 tensor (entries are 1..255)
        _table_cache[key] = (qy, qc, torch.tensor(qy, dtype=torch.int16, device=device), torch.tensor(qc, dtype=torch.int16, device=device))
    return _table_cache[key]


def _check_video(shape, dtype_ok: bool, dtype) -> None:
    if not dtype_ok or len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f"write_mjpeg_avi: video must be uint8 (T, H, W, 3), got {dtype} {tuple(shape)}")


def encode_jpeg_frames(frames, quality: int = 95) -> List[bytes]:
    """uint8 (T, H, W, 3) frames (a device tensor; anything else is uploaded) -> T complete JPEG files, encoded on the device.

    Baseline sequential JPEG, 4:4:4 (see the module docstring for why not 4:2:0), libjpeg's tables for `quality`, the Annex K
    Huffman tables.  Two entry points (ops.jpeg_quantize, ops.jpeg_pack: four launches), then two copies to the host: the T
    byte counts, and the packed streams cut to the longest of them.  FF stuffing (`bytes.replace`) and the markers happen here.
    H and W must be multiples of 8."""
    from . import ops

    if not torch.cuda.is_available():
        raise RuntimeError(f"encode_jpeg_frames: {_NEEDS_GPU}")
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[0] == 0:
        raise ValueError(f"encode_jpeg_frames: frames must be a non-empty uint8 (T, H, W, 3), got {frames.dtype} {tuple(frames.shape)}")
    T, H, W, _ = frames.shape
    if H % 8 or W % 8:
        raise ValueError(f"encode_jpeg_frames: H and W must be multiples of 8 (4:4:4, whole MCUs only), got {H} x {W}")
    if not frames.is_cuda:
        frames = frames.cuda()
    qy, qc, qy_d, qc_d = _device_tables(quality, frames.device)
    stream, nbytes = ops.jpeg_pack(ops.jpeg_quantize(frames.detach().contiguous(), qy_d, qc_d))
    counts = nbytes.cpu().tolist()
    packed = stream[:, :max(counts)].cpu().numpy()
    head = _jpeg_header(H, W, qy, qc)
    return [head + packed[t, :counts[t]].tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9" for t in range(T)]


_warned_size = False


def write_mjpeg_avi(filename: str, video_array, fps: float, audio_array=None, audio_fps: int = 16000, quality: int = 95,
                    encoder: Optional[str] = None) -> str:
    """`encoder`: "host" (PIL) or "device" (`encode_jpeg_frames`); None = the `set_jpeg_encoder` setting.  "device" uploads a host
    array first, needs a GPU, and leaves frames whose H or W is no multiple of 8 to PIL (with one warning)."""
    global _warned_size
    mode = _jpeg_encoder if encoder is None else encoder
    if mode not in _JPEG_ENCODERS:
        raise ValueError(f"write_mjpeg_avi: unknown encoder {mode!r}; one of {_JPEG_ENCODERS}")
    frames = None
    if mode == "device":
        if not torch.cuda.is_available():
            raise RuntimeError(f'write_mjpeg_avi(encoder="device"): {_NEEDS_GPU}')
        v = video_array if torch.is_tensor(video_array) else np.asarray(video_array)
        _check_video(v.shape, v.dtype == (torch.uint8 if torch.is_tensor(v) else np.uint8), v.dtype)
        T, H, W, _ = v.shape
        if H % 8 or W % 8:
            if not _warned_size:
                warnings.warn(f"write_mjpeg_avi: the device JPEG encoder takes frames whose height and width are multiples of 8, got "
                              f"{H} x {W}: PIL encodes these (4:2:0)", RuntimeWarning, stacklevel=2)
                _warned_size = True
        else:
            frames = encode_jpeg_frames(v, quality)
    if frames is None:
        from PIL import Image

        video = video_array.detach().cpu().numpy() if torch.is_tensor(video_array) else np.asarray(video_array)
        _check_video(video.shape, video.dtype == np.uint8, video.dtype)
        T, H, W, _ = video.shape
        frames = []
        for t in range(T):
            buf = io.BytesIO()
            Image.fromarray(video[t]).save(buf, format="JPEG", quality=quality)
            frames.append(buf.getvalue())
    pcm, nch = b"", 0
    if audio_array is not None:
        a = audio_array.detach().cpu().numpy() if torch.is_tensor(audio_array) else np.asarray(audio_array)
        if a.ndim == 1:
            a = a[None]
        nch = a.shape[0]
        pcm = (np.clip(a.T.astype(np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2").tobytes()      # interleaved
    rate, scale = int(round(fps * 1000)), 1000
    max_frame = max(len(f) for f in frames)
    streams = 1 + (1 if nch else 0)
    avih = struct.pack("<14I", int(round(1e6 / fps)), 0, 0, 0x10, T, 0, streams, max_frame, W, H, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, T, max_frame, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
    if nch:
        align = 2 * nch
        nsamp = len(pcm) // align
        strh_a = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, audio_fps * align, 0, nsamp, len(pcm), 0xFFFFFFFF,
                             align, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, nch, audio_fps, audio_fps * align, align, 16, 0)
        hdrl += _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
    movi, index, off = b"", b"", 4
    items = [(b"00dc", f) for f in frames] + ([(b"01wb", pcm)] if nch else [])
    for tag, data in items:
        index += struct.pack("<4sIII", tag, 0x10, off, len(data))
        c = _chunk(tag, data)
        movi += c
        off += len(c)
    body = b"AVI " + _list(b"hdrl", hdrl) + _list(b"movi", movi) + _chunk(b"idx1", index)
    with open(filename, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return filename


def read_mjpeg_avi(filename: str) -> Tuple[torch.Tensor, float, Optional[torch.Tensor], int]:
    """-> (video (T, H, W, 3) uint8, fps, audio (C, Ta) float or None, audio_fps) of a file written above."""
    from PIL import Image

    with open(filename, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{filename}: not a RIFF/AVI file")
    frames, pcm, fps, nch, afps = [], b"", 0.0, 0, 16000

    def walk(lo: int, hi: int):
        nonlocal pcm, fps, nch, afps
        p = lo
        while p + 8 <= hi:
            tag, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            body = p + 8
            if tag == b"LIST":
                walk(body + 4, body + n)
            elif tag == b"strh" and data[body:body + 4] == b"vids":
                scale, rate = struct.unpack("<II", data[body + 20:body + 28])
                fps = rate / scale
            elif tag == b"strf" and n == 18:
                _, nch, afps = struct.unpack("<HHI", data[body:body + 8])
            elif tag == b"00dc":
                frames.append(np.array(Image.open(io.BytesIO(data[body:body + n])).convert("RGB")))
            elif tag == b"01wb":
                pcm += data[body:body + n]
            p = body + n + (n & 1)

    walk(12, len(data))
    video = torch.from_numpy(np.stack(frames))
    audio = None
    if nch:
        audio = torch.from_numpy(np.frombuffer(pcm, dtype="<i2").reshape(-1, nch).T.astype(np.float32) / 32767.0)
    return video, fps, audio, afps
