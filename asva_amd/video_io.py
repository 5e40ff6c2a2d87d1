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
import re
import struct
import warnings
from typing import List, Optional, Sequence, Tuple

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


def _encode_mjpeg_frames(video_array, quality: int, encoder: Optional[str]) -> Tuple[List[bytes], int, int]:
    """uint8 (T, H, W, 3) frames -> (T complete JPEG files, H, W), by PIL or on the device (see `write_mjpeg_avi`)"""
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
                              f"{H} x {W}: PIL encodes these (4:2:0)", RuntimeWarning, stacklevel=3)
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
    return frames, H, W


def _pcm16(audio_array) -> Tuple[bytes, int]:
    """(C, Ta) or (Ta,) float waveform in [-1, 1] -> (interleaved 16-bit PCM, channels); None -> (b"", 0)"""
    if audio_array is None:
        return b"", 0
    a = audio_array.detach().cpu().numpy() if torch.is_tensor(audio_array) else np.asarray(audio_array)
    if a.ndim == 1:
        a = a[None]
    return (np.clip(a.T.astype(np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2").tobytes(), a.shape[0]


def _avi_hdrl(fps: float, T: int, H: int, W: int, max_frame: int, nch: int, audio_fps: int, pcm_bytes: int) -> bytes:
    """payload of the `hdrl` list: main header, the MJPG stream and, with nch > 0, the PCM stream"""
    rate, scale = int(round(fps * 1000)), 1000
    streams = 1 + (1 if nch else 0)
    avih = struct.pack("<14I", int(round(1e6 / fps)), 0, 0, 0x10, T, 0, streams, max_frame, W, H, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, T, max_frame, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
    if nch:
        align = 2 * nch
        nsamp = pcm_bytes // align
        strh_a = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, audio_fps * align, 0, nsamp, pcm_bytes, 0xFFFFFFFF,
                             align, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, nch, audio_fps, audio_fps * align, align, 16, 0)
        hdrl += _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
    return hdrl


def write_mjpeg_avi(filename: str, video_array, fps: float, audio_array=None, audio_fps: int = 16000, quality: int = 95,
                    encoder: Optional[str] = None) -> str:
    """`encoder`: "host" (PIL) or "device" (`encode_jpeg_frames`); None = the `set_jpeg_encoder` setting.  "device" uploads a host
    array first, needs a GPU, and leaves frames whose H or W is no multiple of 8 to PIL (with one warning)."""
    frames, H, W = _encode_mjpeg_frames(video_array, quality, encoder)
    T = len(frames)
    pcm, nch = _pcm16(audio_array)
    max_frame = max(len(f) for f in frames)
    hdrl = _avi_hdrl(fps, T, H, W, max_frame, nch, audio_fps, len(pcm))
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


class MjpegAviWriter:
    """`write_mjpeg_avi` for videos that arrive in pieces (AudioCondAnimationPipeline.animate_track's windows): `append` encodes
    and writes a piece's frames at once, so a long track never holds more than one piece; `close(audio)` writes the audio chunk
    and the index, then goes back and fills in the headers (frame count, largest frame, audio length), which is all it kept.

        w = MjpegAviWriter(path, fps, (H, W), audio_fps)
        w.append(frames_0); w.append(frames_1); ...          # uint8 (T_i, H, W, 3), host or device
        w.close(audio)                                       # (C, Ta) float waveform or None

    The file is what `read_mjpeg_avi` / `walk_mjpeg_avi` read.  It differs from `write_mjpeg_avi`'s bytes for the same content in
    one place: room for the audio stream's header is set aside before the first frame, and a file closed without audio carries
    a JUNK chunk there instead.  `encoder`: as `write_mjpeg_avi`."""

    def __init__(self, path: str, fps: float, size: Tuple[int, int], audio_fps: int = 16000, quality: int = 95,
                 encoder: Optional[str] = None):
        self.path, self.fps, (self.H, self.W), self.audio_fps = path, float(fps), (int(size[0]), int(size[1])), int(audio_fps)
        self.quality, self.encoder = quality, encoder
        self.n_frames, self._max_frame, self._index = 0, 0, []
        self._room = len(_list(b"hdrl", _avi_hdrl(self.fps, 0, self.H, self.W, 0, 1, self.audio_fps, 0)))
        self._f = open(path, "wb")
        self._f.write(b"\0" * (12 + self._room) + b"LIST\0\0\0\0movi")
        self._off = 4                                     # of the next chunk, from the `movi` tag (what idx1 counts from)

    def _put(self, tag: bytes, data: bytes) -> None:
        self._index.append(struct.pack("<4sIII", tag, 0x10, self._off, len(data)))
        c = _chunk(tag, data)
        self._f.write(c)
        self._off += len(c)

    def append(self, frames) -> int:
        """uint8 (T, H, W, 3) frames (host array, host or device tensor) -> the number of frames in the file so far"""
        if self._f is None:
            raise ValueError("MjpegAviWriter.append: the file is closed")
        if tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"MjpegAviWriter.append: frames must be (T, {self.H}, {self.W}, 3), got {tuple(frames.shape)}")
        jpegs, _, _ = _encode_mjpeg_frames(frames, self.quality, self.encoder)
        for j in jpegs:
            self._put(b"00dc", j)
            self._max_frame = max(self._max_frame, len(j))
        self.n_frames += len(jpegs)
        return self.n_frames

    def close(self, audio=None) -> str:
        if self._f is None:
            return self.path
        if self.n_frames == 0:
            self._f.close()
            self._f = None
            raise ValueError("MjpegAviWriter.close: no frames were appended")
        pcm, nch = _pcm16(audio)
        if nch:
            self._put(b"01wb", pcm)
        movi_bytes = self._off                            # `movi` tag + chunks
        self._f.write(_chunk(b"idx1", b"".join(self._index)))
        total = self._f.tell()
        head = _list(b"hdrl", _avi_hdrl(self.fps, self.n_frames, self.H, self.W, self._max_frame, nch, self.audio_fps, len(pcm)))
        if len(head) < self._room:
            head += _chunk(b"JUNK", b"\0" * (self._room - len(head) - 8))
        assert len(head) == self._room
        self._f.seek(0)
        self._f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + head + b"LIST" + struct.pack("<I", movi_bytes))
        self._f.close()
        self._f = None
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self._f is not None:
            self._f.close()
            self._f = None


# ---- where the frames are decoded ----------------------------------------------------------------------------------------
_JPEG_DECODERS = ("host", "device")
_jpeg_decoder = "host"
_DEC_NEEDS_GPU = ('the "device" JPEG decoder needs the GPU (torch.cuda.is_available() is False) and has no host path; '
                  'use "host"')


def set_jpeg_decoder(mode: str) -> None:
    """Who decodes the frames `read_mjpeg_avi` and the clip loaders (data_utils._MjpegClip) return.  "host": PIL, host tensors,
    the default.  "device": `decode_jpeg_frames` (avsd_jpeg_decode_scan + avsd_jpeg_idct_rgb_u8), device tensors; needs a GPU.
    Read once from $AVSD_JPEG_DECODER at import."""
    global _jpeg_decoder
    if mode not in _JPEG_DECODERS:
        raise ValueError(f"set_jpeg_decoder: unknown mode {mode!r}; one of {_JPEG_DECODERS}")
    if mode == "device" and not torch.cuda.is_available():
        raise RuntimeError(f'set_jpeg_decoder("device"): {_DEC_NEEDS_GPU}')
    _jpeg_decoder = mode


def get_jpeg_decoder() -> str:
    return _jpeg_decoder


def _decoder_from_env(environ=os.environ) -> None:
    if environ.get("AVSD_JPEG_DECODER"):
        set_jpeg_decoder(environ["AVSD_JPEG_DECODER"])


_decoder_from_env()

_NEXT_MARKER = re.compile(rb"\xff[^\x00\xff]")


def parse_jpeg(data: bytes) -> dict:
    """The markers of one JPEG file, for the device decoder -> {"H", "W", "sampling": "444" | "420", "qtabs": the three components'
    quantisation tables (64 entries each, zigzag order, as bytes), "huff": the three components' ((DC BITS, HUFFVAL), (AC BITS,
    HUFFVAL)) as bytes, "scan": the entropy-coded segment with its FF 00 stuffing}.  Accepts SOI, APPn / COM, DQT with 8-bit
    entries, SOF0 with 8-bit samples and three components sampled (1x1, 1x1, 1x1) or (2x2, 1x1, 1x1), DHT, DRI of 0, one
    interleaved SOS with Ss = 0, Se = 63, Ah = Al = 0, EOI.  Anything else raises ValueError naming what was found."""
    def bad(what):
        return ValueError(f"parse_jpeg: {what}; the device decoder takes baseline JPEG with three components, 4:4:4 or 4:2:0, one scan, "
                          "no restart interval")

    if data[:2] != b"\xff\xd8":
        raise bad(f"the file starts with {bytes(data[:2]).hex()}, not with SOI")
    p, dqt, dht, sof, sos = 2, {}, {}, None, None
    while sos is None:
        if p + 4 > len(data):
            raise bad("the file ends before SOS")
        if data[p] != 0xFF:
            raise bad(f"byte {data[p]:#04x} at {p} where a marker was expected")
        m = data[p + 1]
        if m == 0xFF:                                             # fill byte
            p += 1
            continue
        n = struct.unpack(">H", data[p + 2:p + 4])[0]
        seg = data[p + 4:p + 2 + n]
        if n < 2 or len(seg) != n - 2:
            raise bad(f"segment {m:#04x} at {p} is cut short")
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4 or len(seg) < q + 65:
                    raise bad("a quantisation table with 16-bit entries" if seg[q] >> 4 else "a DQT segment that is cut short")
                dqt[seg[q] & 15] = bytes(seg[q + 1:q + 65])
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                bits = bytes(seg[q + 1:q + 17])
                cnt = sum(bits)
                if len(bits) != 16 or cnt > 256 or len(seg) < q + 17 + cnt or seg[q] & 0xEE:
                    raise bad(f"a DHT segment that is cut short or names table {seg[q]:#04x}")
                dht[seg[q]] = (bits, bytes(seg[q + 17:q + 17 + cnt]))
                q += 17 + cnt
        elif m == 0xC0:
            if len(seg) < 6 or seg[0] != 8 or seg[5] != 3 or len(seg) != 15:
                raise bad(f"SOF0 with {seg[0] if seg else '?'}-bit samples and {seg[5] if len(seg) > 5 else '?'} component(s)")
            sof = seg
        elif m == 0xDD:
            if len(seg) != 2 or seg[0] or seg[1]:
                raise bad(f"a restart interval (DRI {struct.unpack('>H', seg[:2])[0] if len(seg) >= 2 else '?'})")
        elif m == 0xDA:
            if sof is None:
                raise bad("SOS before SOF0")
            if len(seg) != 10 or seg[0] != 3 or bytes(seg[7:10]) != b"\x00\x3f\x00":
                raise bad(f"a scan of {seg[0] if seg else '?'} component(s) with Ss, Se, AhAl = {bytes(seg[-3:]).hex()} (not one interleaved "
                          "sequential scan)")
            sos = seg
        elif 0xC1 <= m <= 0xCF:
            name = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding",
                    0xCB: "arithmetic coding", 0xCC: "arithmetic coding (DAC)"}.get(m, "differential / arithmetic")
            raise bad(f"marker {m:#04x}: {name}")
        else:
            raise bad(f"marker {m:#04x} at {p}")
        p += 2 + n
    H, W = struct.unpack(">HH", sof[1:5])
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i], sof[8 + 3 * i]) for i in range(3)]
    samp = tuple(c[1] for c in comps)
    if samp not in ((0x11, 0x11, 0x11), (0x22, 0x11, 0x11)):
        raise bad("sampling factors " + ", ".join(f"{s >> 4}x{s & 15}" for s in samp))
    if H < 1 or W < 1:
        raise bad(f"a frame of {H} x {W}")
    qtabs, huff = [], []
    for i, (cid, _s, tq) in enumerate(comps):
        if sos[1 + 2 * i] != cid:
            raise bad("a scan whose components are not in the frame's order")
        td, ta = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
        if tq not in dqt or td not in dht or (0x10 | ta) not in dht:
            raise bad(f"component {i} refers to a table that is missing (quantisation {tq}, DC {td}, AC {ta})")
        qtabs.append(dqt[tq])
        huff.append((dht[td], dht[0x10 | ta]))
    m = _NEXT_MARKER.search(data, p)
    if m is None:
        raise bad("no EOI behind the scan")
    if data[m.start() + 1] != 0xD9:
        raise bad(f"marker {data[m.start() + 1]:#04x} inside or behind the scan (restart markers or a further scan)")
    return {"H": H, "W": W, "sampling": "444" if samp[0] == 0x11 else "420", "qtabs": tuple(qtabs), "huff": tuple(huff),
            "scan": bytes(data[p:m.start()])}


def huffman_decode_table(bits: bytes, vals: bytes, dc: bool) -> np.ndarray:
    """(BITS, HUFFVAL) -> the 352 words of avsd.h: lut[256], limit[16], offset[16], vals[64]; codes by the procedure of Annex C"""
    out = np.zeros(352, dtype=np.uint32)
    code, k = 0, 0
    for length in range(1, 17):
        cnt = bits[length - 1]
        out[272 + length - 1] = (k - code) & 0xFFFFFFFF
        if length <= 8:
            for _ in range(cnt):
                lo = code << (8 - length)
                out[lo:lo + (1 << (8 - length))] = (length << 8) | vals[k]
                code += 1
                k += 1
        else:
            code += cnt
            k += cnt
        if code > 1 << length:
            raise ValueError("parse_jpeg: a Huffman table with more codes than its lengths allow")
        out[256 + length - 1] = code << (16 - length)
        code <<= 1
    if dc and any(v > 11 for v in vals):
        raise ValueError(f"parse_jpeg: a DC Huffman table with category {max(vals)} (baseline has 0..11)")
    out[288:] = np.frombuffer(bytes(vals).ljust(256, b"\0"), dtype="<u4")
    return out


_dec_cache = {}


def _decode_tables(key, build, device):
    """one upload per distinct table set and device"""
    k = (key, str(device))
    if k not in _dec_cache:
        if len(_dec_cache) > 256:
            _dec_cache.clear()
        _dec_cache[k] = build()
    return _dec_cache[k]


def _stack(ts):
    return ts[0][None] if len(ts) == 1 else torch.stack(ts)


JPEG_STATUS = {1: "a code no table assigns", 2: "more blocks than the frame has", 4: "a run behind coefficient 63",
               8: "the scan ends before the last block", 16: "bits left over behind the last block", 32: "arguments out of range"}


def _entropy_decode(jpegs, device, subseq_bits, counters, infos):
    """parse, unstuff, upload, avsd_jpeg_decode_scan -> (H, W, sampling, coef, status, qtabs, q_index), all tensors on the device"""
    from . import ops

    if not torch.cuda.is_available():
        raise RuntimeError(f"decode_jpeg_frames: {_DEC_NEEDS_GPU}")
    if len(jpegs) == 0:
        raise ValueError("decode_jpeg_frames: no frames")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"decode_jpeg_frames: device must be a GPU, got {device}")
    infos = infos or [parse_jpeg(j) for j in jpegs]
    H, W, sampling = infos[0]["H"], infos[0]["W"], infos[0]["sampling"]
    for t, i in enumerate(infos):
        if (i["H"], i["W"], i["sampling"]) != (H, W, sampling):
            raise ValueError(f"decode_jpeg_frames: frame {t} is {i['H']} x {i['W']} {i['sampling']}, frame 0 is {H} x {W} {sampling}; all "
                             "frames of a call have one size and one sampling")
    _, bpm, edge = ops.JPEG_SAMPLINGS[sampling]
    blocks = -(-H // edge) * -(-W // edge) * bpm
    scans = [i["scan"].replace(b"\xff\x00", b"\xff") for i in infos]
    if max(len(sc) for sc in scans) * 8 > 1 << 30:
        raise ValueError("decode_jpeg_frames: a scan longer than 2^30 bits")
    offsets, buf = [], bytearray()
    for sc in scans:
        offsets.append(len(buf))
        buf += sc + b"\xff" * ((-len(sc)) % 8 + 8)                 # 8 bytes the bit reader may touch; 8-byte alignment for what follows
    hkeys, qkeys, hidx, qidx = {}, {}, [], []
    for i in infos:
        hidx.append(hkeys.setdefault(i["huff"], len(hkeys)))
        qidx.append(qkeys.setdefault(i["qtabs"], len(qkeys)))
    htabs = _stack([_decode_tables(("h", k), lambda k=k: torch.from_numpy(np.concatenate(
        [huffman_decode_table(*spec, dc=(j == 0)) for comp in k for j, spec in enumerate(comp)]).view(np.int32)).to(device), device) for k in hkeys])
    qtabs = _stack([_decode_tables(("q", k), lambda k=k: torch.tensor([list(q) for q in k], dtype=torch.int16, device=device), device)
                    for k in qkeys])
    T, n_scan = len(jpegs), len(buf)
    buf += np.asarray(offsets, dtype="<i8").tobytes()              # the scans and the per-frame words: one upload
    buf += np.asarray([8 * len(sc) for sc in scans] + hidx + qidx, dtype="<i4").tobytes()
    up = torch.frombuffer(buf, dtype=torch.uint8).to(device)
    words = up[n_scan + 8 * T:].view(torch.int32)
    coef, status, *rounds = ops.jpeg_decode_scan(up[:n_scan], up[n_scan:n_scan + 8 * T].view(torch.int64), words[:T], words[T:2 * T], htabs, blocks,
                                                 sampling, subseq_bits or ops.JPEG_SUBSEQ_BITS, return_rounds=counters is not None)
    if counters is not None:
        counters["upload_bytes"] = len(buf)
        counters["rounds"] = rounds[0]
    return H, W, sampling, coef, status, qtabs, words[2 * T:3 * T]


def _check_status(status, counters) -> None:
    """the one copy back: the status words (and the round counters, when asked for)"""
    if counters is not None:
        counters["rounds"] = counters["rounds"].cpu().tolist()
    for t, s in enumerate(status.cpu().tolist()):
        if s:
            why = ", ".join(v for b, v in JPEG_STATUS.items() if s & b)
            raise ValueError(f"decode_jpeg_frames: frame {t} did not decode (status {s}: {why})")


def decode_jpeg_coefficients(jpegs: Sequence[bytes], device=None, subseq_bits: Optional[int] = None, counters: Optional[dict] = None) -> torch.Tensor:
    """The first half of `decode_jpeg_frames`: T complete JPEG files -> int16 (T, blocks, 64) on the device, the quantised
    coefficients in zigzag order, blocks in scan order, DC values absolute."""
    _H, _W, _sampling, coef, status, _q, _qi = _entropy_decode(jpegs, device, subseq_bits, counters, None)
    _check_status(status, counters)
    return coef


def decode_jpeg_frames(jpegs: Sequence[bytes], device=None, subseq_bits: Optional[int] = None, counters: Optional[dict] = None,
                       _infos=None) -> torch.Tensor:
    """T complete JPEG files of one size and one sampling -> uint8 (T, H, W, 3) on the device, decoded there.

    The host parses the markers (`parse_jpeg`: baseline, three components, 4:4:4 or 4:2:0; anything else raises ValueError), removes
    the FF 00 stuffing, concatenates the scans into one padded buffer (one upload, with the per-frame offsets, bit lengths and table
    indices), and builds the Huffman decode tables; quantisation and Huffman tables may differ from frame to frame, each distinct
    set is uploaded once per process.  Two entry points (ops.jpeg_decode_scan, ops.jpeg_idct_rgb: three launches), then one copy to
    the host: the T status words.  A stream that does not decode raises ValueError naming the first such frame.  The pixels are
    the ones PIL returns for the same files.  `subseq_bits`: see ops.jpeg_decode_scan; the result does not depend on it.
    `counters`, if given, receives "upload_bytes" and "rounds" (the re-decoding rounds of each frame, copied back with the status)."""
    from . import ops

    H, W, sampling, coef, status, qtabs, q_index = _entropy_decode(jpegs, device, subseq_bits, counters, _infos)
    frames = ops.jpeg_idct_rgb(coef, H, W, sampling, qtabs, q_index)
    _check_status(status, counters)
    return frames


def walk_mjpeg_avi(filename: str) -> Tuple[List[bytes], float, bytes, int, int]:
    """The container walk of a file written above -> (compressed frames, fps, interleaved 16-bit PCM, channels, audio rate)."""
    with open(filename, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{filename}: not a RIFF/AVI file")
    frames, pcm, fps, nch, afps, codec = [], b"", 0.0, 0, 16000, None

    def walk(lo: int, hi: int):
        nonlocal pcm, fps, nch, afps, codec
        p = lo
        while p + 8 <= hi:
            tag, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            body = p + 8
            if tag == b"LIST":
                walk(body + 4, body + n)
            elif tag == b"strh" and data[body:body + 4] == b"vids":
                codec = data[body + 4:body + 8]
                scale, rate = struct.unpack("<II", data[body + 20:body + 28])
                fps = rate / scale
            elif tag == b"strf" and n == 18:
                _, nch, afps = struct.unpack("<HHI", data[body:body + 8])
            elif tag == b"00dc":
                frames.append(data[body:body + n])
            elif tag == b"01wb":
                pcm += data[body:body + n]
            p = body + n + (n & 1)

    walk(12, len(data))
    if codec is not None and codec.upper() != b"MJPG":
        raise ValueError(f"{filename}: the video stream is {codec!r}, not MJPG")
    return frames, fps, pcm, nch, afps


_warned_format = False


def decode_mjpeg_frames(frames: Sequence[bytes], decoder: Optional[str] = None, device=None) -> torch.Tensor:
    """The decode step: compressed frames -> uint8 (T, H, W, 3).  `decoder`: "host" (PIL, a host tensor) or "device"
    (`decode_jpeg_frames`, a device tensor); None = the `set_jpeg_decoder` setting.  "device" leaves files the device decoder
    refuses (progressive, greyscale, 4:2:2, restart markers, ...) to PIL and uploads the result, with one warning per process."""
    global _warned_format
    mode = _jpeg_decoder if decoder is None else decoder
    if mode not in _JPEG_DECODERS:
        raise ValueError(f"decode_mjpeg_frames: unknown decoder {mode!r}; one of {_JPEG_DECODERS}")
    if mode == "device":
        if not torch.cuda.is_available():
            raise RuntimeError(f'decode_mjpeg_frames(decoder="device"): {_DEC_NEEDS_GPU}')
        try:
            infos = [parse_jpeg(f) for f in frames]
            if len({(i["H"], i["W"], i["sampling"]) for i in infos}) > 1:
                raise ValueError("parse_jpeg: frames of different sizes or samplings in one file")
        except ValueError as e:
            if not _warned_format:
                warnings.warn(f"the device JPEG decoder does not take this file ({e}): PIL decodes it and the frames are uploaded",
                              RuntimeWarning, stacklevel=3)
                _warned_format = True
        else:
            return decode_jpeg_frames(frames, device, _infos=infos)
    from PIL import Image

    video = torch.from_numpy(np.stack([np.array(Image.open(io.BytesIO(f)).convert("RGB")) for f in frames]))
    return video.to(torch.device("cuda" if device is None else device)) if mode == "device" else video


def read_mjpeg_avi(filename: str, decoder: Optional[str] = None, device=None) -> Tuple[torch.Tensor, float, Optional[torch.Tensor], int]:
    """-> (video (T, H, W, 3) uint8, fps, audio (C, Ta) float or None, audio_fps) of a file written above.  `decoder`, `device`: see
    `decode_mjpeg_frames`; with the "host" decoder (the default setting) the video is a host tensor decoded by PIL."""
    frames, fps, pcm, nch, afps = walk_mjpeg_avi(filename)
    video = decode_mjpeg_frames(frames, decoder, device)
    audio = None
    if nch:
        audio = torch.from_numpy(np.frombuffer(pcm, dtype="<i2").reshape(-1, nch).T.astype(np.float32) / 32767.0)
    return video, fps, audio, afps
